"""CPU: CRC-aided GRU list decoding (RNN_decoder.list_decode_crc, npd_gru_list_decode_crc / _crc_mc) -- the selection
rule the tests hold the kernel to, what is refused, and that the GPU tests' inputs exercise every branch of the rule.

  * tests/ca_rnnl_helper.py's ca_choice on hand-made lists: a passing path beats a nearer failing one; with no
    passing path the nearest wins; of two passing paths the nearer; the first in list order on a tie.
  * list_decode_crc needs a CRC on the code, and refuses everything list_decode refuses, before any GPU work.
  * the C entry points reject NULL handles, bad polynomials and bad list sizes; the CLI takes --crc_len with
    --crisp --rnn_list_size.
  * input conditions: on the seeded Polar(32,16) recipe with polynomial 0xB, each of the three word classes (no path
    passes / the plain choice passes / the plain choice fails and another path passes) holds >= 5 % of the 515 words
    at every L in {2, 3, 4, 5, 8}, and no eligible-distance gap is below DIST_MARGIN, in the float64 restatement.
"""
import ctypes

import numpy as np
import pytest

import ca_rnnl_helper as C
import rnnl_helper as H


def _pm(bits):
    return 1.0 - 2.0 * np.asarray(bits, np.float64)


# poly 0xB = x^3 + x + 1: 0001011 is the polynomial itself (remainder 0), as is the all-zero word
PASS_A = [0, 0, 0, 1, 0, 1, 1]
PASS_B = [0, 0, 1, 0, 1, 1, 0]   # x (x^3 + x + 1)
PASS_0 = [0, 0, 0, 0, 0, 0, 0]
FAIL_A = [0, 0, 0, 0, 0, 0, 1]
FAIL_B = [1, 0, 0, 0, 0, 0, 0]


def test_hand_made_words_have_the_remainders_the_cases_assume():
    reg = C.cand_remainders(_pm([[PASS_A, PASS_B, PASS_0, FAIL_A, FAIL_B]]), 0xB)[0]
    assert list(reg[:3]) == [0, 0, 0] and reg[3] == 1 and reg[4] not in (0, -1)


def test_a_passing_path_that_is_not_the_nearest_wins():
    sel, ok, reg = C.ca_choice(_pm([[FAIL_A, PASS_A, FAIL_B]]), [[1.0, 5.0, 2.0]], 0xB)
    assert sel[0] == 1 and ok[0] == 1 and reg[0, 1] == 0


def test_no_passing_path_means_the_nearest_wins():
    sel, ok, _ = C.ca_choice(_pm([[FAIL_A, FAIL_B, FAIL_A]]), [[3.0, 2.0, 2.5]], 0xB)
    assert sel[0] == 1 and ok[0] == 0


def test_of_two_passing_paths_the_nearer_wins():
    sel, ok, _ = C.ca_choice(_pm([[PASS_A, FAIL_A, PASS_B]]), [[5.0, 1.0, 4.0]], 0xB)
    assert sel[0] == 2 and ok[0] == 1


def test_first_in_list_order_on_a_tie():
    sel, ok, _ = C.ca_choice(_pm([[FAIL_A, PASS_B, PASS_A, PASS_0]]), [[1.0, 4.0, 4.0, 4.0]], 0xB)
    assert sel[0] == 1 and ok[0] == 1
    sel, ok, _ = C.ca_choice(_pm([[FAIL_A, FAIL_B]]), [[2.0, 2.0]], 0xB)
    assert sel[0] == 0 and ok[0] == 0


def test_unused_slots_do_not_pass():
    cand = np.concatenate([_pm([[FAIL_A, FAIL_B]]), np.zeros((1, 2, 7))], 1)
    sel, ok, reg = C.ca_choice(cand, [[3.0, 2.0, 0.0, 0.0]], 0xB)
    assert sel[0] == 1 and ok[0] == 0 and list(reg[0, 2:]) == [-1, -1]


def _net(rnn_type="GRU", F=32, layers=2, N=16, onehot=True, **kw):
    from neural_polar_decoder_amd.rnn import RNN_Model
    return RNN_Model(rnn_type, N + 1 + int(onehot), F, 1, layers, N, kw.pop("y_hidden", 0), 0, **kw).eval()


def test_list_decode_crc_needs_a_crc_on_the_code():
    import torch
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.rnn import RNN_decoder
    N, K = 16, 8
    code = reference_polar_code(N, K)
    dec = RNN_decoder("y_input", N, np.asarray(code.info_positions), onehot=True)
    y = torch.zeros(4, N)
    with pytest.raises(ValueError, match="no CRC is set"):
        dec.list_decode_crc(_net(), y, code, 4)
    with pytest.raises(ValueError, match="no CRC is set"):
        dec.list_decode(_net(), y, code, 4, use_CRC=True)
    code.set_crc(3)
    code.set_crc(0)
    with pytest.raises(ValueError, match="no CRC is set"):
        dec.list_decode_crc(_net(), y, code, 4)


def test_list_decode_crc_refuses_what_list_decode_refuses_without_a_gpu():
    import torch
    from neural_polar_decoder_amd import _lib, reference_polar_code
    from neural_polar_decoder_amd.rnn import RNN_decoder
    N, K = 16, 8
    code = reference_polar_code(N, K)
    code.set_crc(3)
    info = np.asarray(code.info_positions)
    y = torch.zeros(4, N)
    cnt = torch.zeros(3, dtype=torch.int64)
    ok = RNN_decoder("y_input", N, info, onehot=True)
    cases = [
        (RNN_decoder("y_h0", N, info, onehot=True), _net(), 4, "y_input"),
        (RNN_decoder("y_input", N, info, onehot=True, reverse_order=True), _net(), 4, "reverse_order"),
        (RNN_decoder("y_input", N, info, onehot=True, precision="fp16x3"), _net(), 4, "fp32"),
        (RNN_decoder("y_input", N, info, onehot=True, precision="bf16"), _net(), 4, "fp32"),
        (ok, _net(bidirectional=True), 4, "unidirectional"),
        (ok, _net("LSTM"), 4, "LSTM"),
        (ok, _net(use_layernorm=True), 4, "LayerNorm"),
        (ok, _net(out_linear_depth=2, y_hidden=32), 4, "out_linear_depth"),
        (ok, _net(F=128), 4, "feature_size"),
        (ok, _net(F=16), 4, "feature_size"),
        (ok, _net(), 0, "list size"),
        (ok, _net(), 9, "list size"),
        (ok, _net(), 2.5, "list size"),
    ]
    for dec, net, L, word in cases:
        with pytest.raises(_lib.NpdError, match=word):
            dec.list_decode_crc(net, y, code, L)
        with pytest.raises(_lib.NpdError, match=word):
            dec.list_decode(net, y, code, L, use_CRC=True)
        with pytest.raises(_lib.NpdError, match=word):
            dec.list_decode_crc_mc(net, y, code, L, 1, 0, cnt)


def test_c_entry_points_reject_null_bad_polynomials_and_bad_list_sizes():
    from neural_polar_decoder_amd import _lib
    from neural_polar_decoder_amd.polar import _CodeHandle
    L = _lib.load()
    one = ctypes.c_void_p(16)  # non-NULL, never dereferenced: every call below fails a check first
    code = _CodeHandle(16, np.arange(8, 16), 0)  # K = 8
    buf = ctypes.create_string_buffer(4096)  # a zeroed handle image (tests/test_rnnl.py): readable, F = 0
    fake = ctypes.cast(buf, ctypes.c_void_p)

    def dec(g, c, y, ls, poly, hat, B, cand=None):
        return L.npd_gru_list_decode_crc(g, c, y, None, ls, poly, hat, None, None, cand, None, None, B, None)

    def mc(g, c, y, ls, poly, B, cnt=one):
        return L.npd_gru_list_decode_crc_mc(g, c, y, None, ls, poly, None, 1, 0, B, cnt, None)

    assert dec(None, code.h, one, 4, 0xB, one, 4) == -1 and b"gru is NULL" in L.npd_last_error()
    assert dec(fake, None, one, 4, 0xB, one, 4) == -1 and b"code is NULL" in L.npd_last_error()
    assert dec(fake, code.h, one, 4, 0xB, one, -1) == -1
    assert mc(None, code.h, one, 4, 0xB, 4) == -1 and b"gru is NULL" in L.npd_last_error()
    assert mc(fake, None, one, 4, 0xB, 4) == -1 and b"code is NULL" in L.npd_last_error()
    assert mc(fake, code.h, one, 4, 0xB, -1) == -1
    assert mc(fake, code.h, one, 4, 0xB, 4, cnt=None) == -1 and b"counters" in L.npd_last_error()
    for bad in (0, 9, -3):
        assert dec(fake, code.h, one, bad, 0xB, one, 4) == -1 and b"list_size" in L.npd_last_error()
        assert mc(fake, code.h, one, bad, 0xB, 4) == -1 and b"list_size" in L.npd_last_error()
    # polynomials against K = 8, on a handle of the code's N: 0 (decode only), bit 0 clear, degree >= K, degree > 24
    ctypes.memmove(buf, ctypes.byref(ctypes.c_int(16)), 4)
    assert dec(fake, code.h, one, 4, 0, one, 4) == -1 and b"crc_poly" in L.npd_last_error()
    for bad in (0xA, 0x1D5, 0x3B2B117, 1):
        assert dec(fake, code.h, one, 4, bad, one, 4) == -1 and b"crc_poly" in L.npd_last_error()
        assert mc(fake, code.h, one, 4, bad, 4) == -1 and b"crc_poly" in L.npd_last_error()
    # a good polynomial (and, for the counting entry point, none) reaches the handle check: not an fp32 list handle
    assert dec(fake, code.h, one, 4, 0xB, one, 4) == -2 and b"fp32" in L.npd_last_error()
    assert mc(fake, code.h, one, 4, 0xB, 4) == -2
    assert mc(fake, code.h, one, 4, 0, 4) == -2
    # the code's N differs from the handle's
    ctypes.memmove(buf, ctypes.byref(ctypes.c_int(32)), 4)
    assert dec(fake, code.h, one, 4, 0xB, one, 4) == -1 and mc(fake, code.h, one, 4, 0xB, 4) == -1


def test_cli_takes_crc_len_with_the_gru_list():
    from neural_polar_decoder_amd import montecarlo
    a = montecarlo._parse_args(["--crisp", "--rnn_list_size", "4", "--crc_len", "3", "--N", "32", "--K", "16"])
    assert a.crc_len == 3 and a.rnn_list_size == 4 and a.crisp and a.list_size is None
    a = montecarlo._parse_args(["--list_size", "8", "--crisp", "--rnn_list_size", "8", "--crc_len", "8"])
    assert a.crc_len == 8 and a.list_size == 8 and a.rnn_list_size == 8
    assert montecarlo._parse_args(["--list_size", "8", "--crc_len", "8"]).crc_len == 8
    with pytest.raises(SystemExit):
        montecarlo._parse_args(["--crc_len", "8"])                      # alone
    with pytest.raises(SystemExit):
        montecarlo._parse_args(["--crisp", "--crc_len", "8"])           # --crisp without a list
    with pytest.raises(SystemExit):
        montecarlo._parse_args(["--rnn_list_size", "4", "--crc_len", "8"])  # --rnn_list_size needs --crisp
    with pytest.raises(SystemExit):
        montecarlo._parse_args(["--crisp", "--rnn_list_size", "4", "--crc_len", "8", "--K", "8"])  # no message bit left
    assert issubclass(montecarlo.CAGRUListMonteCarlo, montecarlo.GRUListMonteCarlo)
    with pytest.raises(ValueError, match="CRC"):
        from neural_polar_decoder_amd import reference_polar_code
        montecarlo.CAGRUListMonteCarlo(reference_polar_code(16, 8), None, None, 4, [0.0], 1, 1, device="cpu")


def test_signatures_hold_the_two_entry_points():
    from neural_polar_decoder_amd import _lib
    names = {s[0]: s for s in _lib.SIGNATURES}
    assert len(names["npd_gru_list_decode_crc"][2]) == 14 and len(names["npd_gru_list_decode_crc_mc"][2]) == 12


@pytest.mark.parametrize("L", [2, 3, 4, 5, 8])
def test_input_conditions_hold_on_the_float64_restatement(L):
    """The seeded Polar(32,16) recipe with polynomial 0xB: every branch of the selection rule is taken by >= 5 % of
    the words, and every eligible-distance gap is clear of the fp32 distance tolerance."""
    from neural_polar_decoder_amd import reference_polar_code
    code = reference_polar_code(32, 16)
    info = np.sort(np.asarray(code.info_positions))
    sd = C.seeded_scaled_state_dict(code, 64, 1, False)
    y = C.seeded_words(32, 16, info)
    r = C.ca_list_decode_np(sd, 32, info, False, 1, y, L, 0xB)
    none, plain, other = C.classes(r["cand_crc"], r["plain_sel"])
    print(f"L = {L}: no path passes {none:.3f}, plain choice passes {plain:.3f}, another path passes {other:.3f}, "
          f"smallest eligible gap {r['elig_gap'].min():.3e}")
    assert min(none, plain, other) >= 0.05
    assert r["elig_gap"].min() >= H.DIST_MARGIN
    # the rule, restated on its own outputs
    rows = np.arange(len(y))
    ok = r["crc_ok"] == 1
    assert np.array_equal(ok, (r["cand_crc"] == 0).any(1))
    assert (r["cand_crc"][rows, r["sel"]][ok] == 0).all()
    assert np.array_equal(r["sel"][~ok], r["plain_sel"][~ok])
    plain_ok = r["cand_crc"][rows, r["plain_sel"]] == 0
    assert np.array_equal(r["sel"][plain_ok], r["plain_sel"][plain_ok])
