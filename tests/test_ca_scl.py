"""CRC-aided SC-List decoding without a GPU: the fp32 restatement (tests/ca_scl_ref.py) against the reference's own
CRC helpers (tests/golden/crc_ref.npz, written by tests/golden/gen_crc.py) and, with the ML rule on its final list,
against the reference's SC-List fixtures; the word sets the GPU tests decode (built on the host, so what they must
exercise is checked here); and the Python / C surface's argument checks.

Bars: exact (bits, and fp32 operations in a fixed order)."""
import ctypes

import numpy as np
import pytest
import torch

from ca_scl_ref import (ALL_SETS, PAC_SETS, POLAR_SETS, QUANT_SETS, case, crc_attach, crc_bits, crc_degree, crc_passes,
                        list_passes, ml_choice, pick, scl_list, set_id)
from conftest import golden

ML_FIXTURES = ["scl_8_4_L4", "scl_16_8_L2", "scl_32_16_L3", "scl_64_32_L8", "pac_scl_32_16_L4", "pac_scl_64_22_L4"]
POLYS = {3: 0xB, 8: 0x1D5, 16: 0x11021, 6: 0x61, 11: 0xE21, 24: 0x1B2B117}


def gf2_divmod_remainder(bits, poly):
    """Remainder of sum bits[k] x^(n-1-k) by the polynomial, by long division on coefficient arrays (numpy)."""
    g = np.array([(poly >> i) & 1 for i in range(crc_degree(poly), -1, -1)], dtype=np.int64)
    r = np.array(bits, dtype=np.int64)
    for k in range(len(r) - len(g) + 1):
        if r[k]:
            r[k:k + len(g)] ^= g
    return r[len(r) - (len(g) - 1):]


def test_crc_reproduces_the_reference_helpers():
    d = golden("crc_ref.npz")
    n = 0
    for c in (3, 8, 16):
        for kc in (1, 5, 8, 24):
            k = f"c{c}_k{kc}"
            poly = int(d[k + "_poly"])
            assert poly == POLYS[c]
            bits, rem = d[k + "_bits"], d[k + "_rem"]
            assert np.array_equal(crc_bits(bits, poly), rem), k
            # CRC_check of [bits, remainder] is 1; of a word with one flipped bit whatever the reference said (0)
            assert d[k + "_check"].all() and not d[k + "_check_flip"].any()
            assert np.array_equal(crc_passes(np.concatenate([bits, rem], 1), poly), d[k + "_check"]), k
            assert np.array_equal(crc_passes(d[k + "_flip"], poly), d[k + "_check_flip"]), k
            n += len(bits)
    assert n == 12 * 24


@pytest.mark.parametrize("c", sorted(POLYS))
def test_crc_is_polynomial_division(c):
    poly = POLYS[c]
    rng = np.random.default_rng(100 + c)
    for kc in (1, 7, 40, 190):
        bits = rng.integers(0, 2, (50, kc))
        r = crc_bits(bits, poly)
        for b, rr in zip(bits, r):
            assert np.array_equal(gf2_divmod_remainder(np.concatenate([b, np.zeros(c, np.int64)]), poly), rr)
        word = np.concatenate([bits, r], 1)
        assert crc_passes(word, poly).all()
        word[np.arange(50), rng.integers(0, kc + c, 50)] ^= 1
        assert not crc_passes(word, poly).any()  # a single error is always detected (bit 0 of the polynomial is set)
    m = 1.0 - 2.0 * rng.integers(0, 2, (5, 9)).astype(np.float32)
    a = crc_attach(m, poly)
    assert a.shape == (5, 9 + c) and np.array_equal(a[:, :9], m) and set(np.unique(a[:, 9:])) <= {-1.0, 1.0}


@pytest.mark.parametrize("name", ML_FIXTURES)
def test_list_with_the_ml_rule_reproduces_the_reference_fixtures(name):
    """Ties the restatement's list to the reference: the ML rule on the whole final list gives the fixture's msg_hat."""
    d = golden(f"{name}.npz")
    g = int(d["g"]) if "g" in d.files else 2
    for s in np.unique(d["snr"]):
        m = d["snr"] == s
        lst = scl_list(d["y"][m], float(s), d["info"], g, int(d["L"]))
        _, vh, uh = pick(lst, ml_choice(lst))
        assert np.array_equal(vh, d["msg_hat"][m]), (name, s)
        if "u_hat" in d.files:
            assert np.array_equal(uh, d["u_hat"][m]), (name, s)


def classes(cs):
    """(a, b, c) word counts: the chosen path is not the list's minimum-metric path / no path passes / some passes."""
    met = cs["lst"]["met"].numpy()
    a = int((cs["best"] != met.argmin(0)).sum())
    return a, int((cs["ok"] == 0).sum()), int((cs["ok"] == 1).sum())


@pytest.mark.parametrize("s", POLAR_SETS + PAC_SETS, ids=lambda s: set_id(s[:6] + (False,)))
def test_word_sets_hold_every_required_class(s):
    cs = case(s[:6] + (False,))
    a, b, c = classes(cs)
    print(set_id(s[:6] + (False,)), "a / b / c =", a, b, c)
    need = s[6]
    assert cs["y"].shape[0] == (333 if s[0] <= 64 else 77)
    assert c >= 3
    if "a" in need:
        assert a >= 3
    if "b" in need:
        assert b >= 3
    # a transmitted word that survives in the list passes: crc_ok = 0 implies the message is not in the list
    sent = (cs["lst"]["v"].numpy()[:, :, cs["info"]] == cs["msg"][None]).all(2).any(0)
    assert not (sent & (cs["ok"] == 0)).any()


@pytest.mark.parametrize("s", QUANT_SETS, ids=lambda s: set_id(s + (True,)))
def test_quantised_sets_hold_zero_decisions_and_metric_ties(s):
    cs = case(s + (True,))
    lst = cs["lst"]
    met = lst["met"].numpy()
    zero = (lst["u"].numpy() == 0).any(2).any(0)
    tie = (met == met.min(0)[None]).sum(0) > 1
    none_tie = (cs["ok"] == 0) & tie
    print(set_id(s + (True,)), "zero decision:", int(zero.sum()), "no pass and min-metric tie:", int(none_tie.sum()))
    assert cs["y"].shape[0] == 200 and np.array_equal(cs["y"], np.round(2 * cs["y"]) / 2)
    assert zero.sum() >= 10 and none_tie.sum() >= 10
    # a path with a zero decision never passes
    ok = list_passes(lst, cs["poly"])
    assert not (ok.astype(bool) & (lst["v"].numpy()[:, :, cs["info"]] == 0).any(2)).any()


def test_all_sets_are_distinct():
    assert len(set(ALL_SETS)) == len(ALL_SETS) == 30


def _codes():
    from neural_polar_decoder_amd import PAC, reference_polar_code
    return [reference_polar_code(32, 16), PAC(None, 32, 16, 53)]


def test_set_crc_argument_errors():
    for code in _codes():
        assert code.CRC_len == 0 and set(code.CRC_polynomials.items()) == set(POLYS.items())
        for c, p in POLYS.items():
            if c < 16:
                code.set_crc(c)
                assert (code.CRC_len, code.crc_poly, code.K_minus_CRC) == (c, p, 16 - c)
        code.set_crc(5, 0x25)
        assert (code.CRC_len, code.crc_poly, code.K_minus_CRC) == (5, 0x25, 11)
        bad = [(5, None), (16, None), (24, None), (8, 0xB), (3, 0xA), (-1, None), (25, 1 << 25 | 1), (3, 0x1D5),
               (0, 0xB), (32, (1 << 32) | 1)]
        for c, p in bad:
            with pytest.raises(ValueError):
                code.set_crc(c, p)
        assert code.CRC_len == 5, "a refused set_crc changes nothing"
        code.set_crc(0)
        assert (code.CRC_len, code.crc_poly, code.K_minus_CRC) == (0, 0, 16)
        with pytest.raises(ValueError):
            code.crc_attach(torch.zeros(2, 8))
        with pytest.raises(ValueError):
            code.scl_decode_crc(torch.zeros(2, 32), 1.0, 4)
        with pytest.raises(ValueError):
            code.mc_generate_crc(4, 1.0, 1)


def test_use_crc_without_a_crc_raises():
    for code in _codes():
        with pytest.raises(NotImplementedError, match="set_crc"):
            code.scl_decode(torch.zeros(4, 32), 1.0, 4, use_CRC=True)
        code.set_crc(8)
        code.set_crc(0)
        with pytest.raises(NotImplementedError, match="set_crc"):
            code.scl_decode(torch.zeros(4, 32), 1.0, 4, use_CRC=True)


def test_cli_parses_crc_len():
    from neural_polar_decoder_amd import montecarlo
    a = montecarlo._parse_args(["--list_size", "8", "--crc_len", "8"])
    assert a.crc_len == 8 and a.list_size == 8
    assert montecarlo._parse_args(["--code", "pac", "--list_size", "4", "--crc_len", "11"]).crc_len == 11
    assert montecarlo._parse_args(["--list_size", "4"]).crc_len is None
    with pytest.raises(SystemExit):
        montecarlo._parse_args(["--crc_len", "8"])                       # needs --list_size
    with pytest.raises(SystemExit):
        montecarlo._parse_args(["--list_size", "4", "--crc_len", "5"])   # not a table length
    with pytest.raises(SystemExit):
        montecarlo._parse_args(["--K", "8", "--list_size", "4", "--crc_len", "8"])  # no message bit left


def test_entry_points_reject_null_and_bad_polynomials():
    """The four entry points refuse NULL operands (with a valid polynomial) and every polynomial the header excludes
    (with valid operands), before any HIP call: no GPU is needed, and nothing is written."""
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    info = np.arange(16, 32, dtype=np.int32)
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    for g in (0, 53):
        h = ctypes.c_void_p()
        assert L.npd_code_create(32, 16, info.ctypes.data_as(ctypes.c_void_p), g, 1000.0, ctypes.byref(h)) == 0
        ok = 0x1D5
        # NULL operands, valid polynomial
        assert L.npd_scl_decode_crc(None, p, 1.0, 4, ok, p, p, p, 4, None) == -1
        assert L.npd_scl_decode_crc(h, None, 1.0, 4, ok, p, p, p, 4, None) == -1
        assert L.npd_scl_decode_crc(h, p, 1.0, 4, ok, None, None, None, 4, None) == -1 and b"no output" in L.npd_last_error()
        assert L.npd_scl_decode_crc_mc(None, p, 1.0, 4, ok, p, 1, 0, 4, p, None) == -1
        assert L.npd_scl_decode_crc_mc(h, None, 1.0, 4, ok, p, 1, 0, 4, p, None) == -1
        assert L.npd_scl_decode_crc_mc(h, p, 1.0, 4, ok, p, 1, 0, 4, None, None) == -1
        assert L.npd_mc_generate_crc(None, ok, p, p, p, 4, 1.0, 1, 0, 0, None) == -1
        assert L.npd_mc_generate_crc(h, ok, p, p, None, 4, 1.0, 1, 0, 0, None) == -1
        assert L.npd_crc_attach(None, p, 4, 16, ok, None) == -1
        assert L.npd_crc_attach(p, None, 4, 16, ok, None) == -1
        # list size and negative batch
        assert L.npd_scl_decode_crc(h, p, 1.0, 0, ok, p, p, p, 4, None) == -1
        assert L.npd_scl_decode_crc(h, p, 1.0, 33, ok, p, p, p, 4, None) == -1
        assert L.npd_scl_decode_crc(h, p, 1.0, 4, ok, p, p, p, -1, None) == -1
        # polynomials: 0, degree 0, bit 0 clear, degree 25, degree >= K (16)
        for bad in (0, 1, 0x1D4, (1 << 25) | 1, 0x11021, (1 << 31) | 1):
            assert L.npd_scl_decode_crc(h, p, 1.0, 4, bad, p, p, p, 4, None) == -1 and b"crc_poly" in L.npd_last_error()
            assert L.npd_scl_decode_crc_mc(h, p, 1.0, 4, bad, p, 1, 0, 4, p, None) == -1
            assert L.npd_mc_generate_crc(h, bad, p, p, p, 4, 1.0, 1, 0, 0, None) == -1
            assert L.npd_crc_attach(p, p, 4, 16, bad, None) == -1 and b"crc_poly" in L.npd_last_error()
        # an empty batch is fine, with or without pointers
        assert L.npd_scl_decode_crc(h, None, 1.0, 4, ok, p, None, None, 0, None) == 0
        assert L.npd_scl_decode_crc_mc(h, None, 1.0, 4, ok, None, 1, 0, 0, p, None) == 0
        assert L.npd_mc_generate_crc(h, ok, None, None, None, 0, 1.0, 1, 0, 0, None) == 0
        assert L.npd_crc_attach(None, None, 0, 16, ok, None) == 0
        assert L.npd_code_destroy(h) == 0
    assert not buf.any()
