"""CRC-aided GRU list decoding on the MI355X (npd_gru_list_decode_crc / _crc_mc; RNN_decoder.list_decode_crc,
list_decode(use_CRC=True), list_decode_crc_mc; CAGRUListMonteCarlo), with the CRC and the rule of include/npd.h.

The selection is a pure function of the kernel's own candidate list, so on the seeded nets of tests/test_rnnl_gpu.py
(seeded_crisp(seed=11), GRU weights x 3, output Linear x 10, generator seed 5, y = encode(msg) + 0.7 randn), for
L in {1, 2, 3, 4, 5, 8} and B in {1, 7, 33, 515}, the checks are exact:
  1. cand_msg and cand_metric are list_decode(return_candidates=True)'s, bit for bit;
  2. cand_crc is ca_scl_ref.crc_remainder of cand_msg's bits for every candidate, -1 for unused slots;
  3. crc_ok == (cand_crc == 0).any(1);
  4. the chosen candidate is eligible; sel is the float64 first minimum over the eligible candidates wherever the two
     smallest eligible distances differ by >= DIST_MARGIN, and everywhere the chosen distance is within DIST_MARGIN of it;
  5. where crc_ok == 0, sel and msg_hat are plain list_decode's; where plain list_decode's choice passes, sel is it;
  6. msg_hat == cand_msg[b, sel[b]], and the Python method returns its first K - c columns.
Then, on the trained Polar(32,16) net, the float64 restatement (list_decode_np + ca_choice) on words that carry a CRC;
the fused counters against list_decode_crc + count_errors, count for count; the Monte-Carlo driver; graph capture;
B = 0 and the optional outputs.
"""
import argparse
import functools

import numpy as np
import pytest
import torch

import ca_rnnl_helper as C
import rnnl_helper as H
from ca_scl_ref import crc_degree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = [1, 7, 33, 515]
LISTS = [1, 2, 3, 4, 5, 8]


def code_of(N, K, pac_g=0):
    from neural_polar_decoder_amd import PAC, reference_polar_code
    if pac_g:
        code = PAC(argparse.Namespace(target_K=K), N, K, pac_g)
        return code, np.sort(np.asarray(code.B))
    if N <= 32:
        code = reference_polar_code(N, K)
    else:
        from neural_polar_decoder_amd import PolarCode
        from neural_polar_decoder_amd.codes import polar_info_positions
        code = PolarCode(int(np.log2(N)), K, F=np.setdiff1d(np.arange(N), polar_info_positions(N, K, "polar", None)))
    return code, np.sort(np.asarray(code.info_positions))


def encode(code, msg):
    return code.pac_encode(msg) if hasattr(code, "pac_encode") else code.encode_plotkin(msg)


SHAPES = {  # name: (N, K, pac_g, F, layers, onehot, words)
    "polar_32_16_f64_l1": (32, 16, 0, 64, 1, False, 515),
    "polar_64_32_f64_l2": (64, 32, 0, 64, 2, True, 515),
    "pac_32_10_f32_l2": (32, 10, 53, 32, 2, True, 515),
    "polar_256_128_f32_l1": (256, 128, 0, 32, 1, True, 33),
    "polar_256_200_f32_l1": (256, 200, 0, 32, 1, True, 33),
    "polar_16_8_f256_l1": (16, 8, 0, 256, 1, True, 33),
    "polar_8_2_f32_l1": (8, 2, 0, 32, 1, True, 33),
}
_cache = {}


def shape_setup(name):
    """(code, info, net, decoder, y on the device): tests/test_rnnl_gpu.py's seeded recipe, built once per shape."""
    if name not in _cache:
        from neural_polar_decoder_amd.montecarlo import seeded_crisp
        N, K, g, F, layers, onehot, words = SHAPES[name]
        code, info = code_of(N, K, g)
        net, dec = seeded_crisp(code, F, layers, seed=11, device=DEV, onehot=onehot)
        with torch.no_grad():
            for k, p in net.named_parameters():
                p.mul_(3.0 if k.startswith("rnn.") else 10.0)
        gen = torch.Generator().manual_seed(5)
        msg = 1.0 - 2.0 * (torch.rand(words, K, generator=gen) < 0.5).float()
        y = encode(code, msg.to(DEV)) + 0.7 * torch.randn(words, N, generator=gen).to(DEV)
        _cache[name] = (code, info, net, dec, y)
    return _cache[name]


def check_invariants(name, poly, L, batches):
    """Items 1 - 6 of the module docstring; returns the outputs of the last batch size as numpy."""
    code, info, net, dec, y_all = shape_setup(name)
    N, K = SHAPES[name][0], SHAPES[name][1]
    c = crc_degree(poly)
    code.set_crc(c, poly)
    try:
        out = None
        for B in batches:
            y = y_all[:B]
            rows = np.arange(B)
            p_hat, (p_cm, p_ct, p_sel) = dec.list_decode(net, y, code, L, return_candidates=True)
            hat, ok, (cm, ct, sel, reg) = dec.list_decode_crc(net, y, code, L, return_ok=True, return_candidates=True)
            via_kw, (_, _, kw_sel, _) = dec.list_decode(net, y, code, L, return_candidates=True, use_CRC=True)
            assert torch.equal(via_kw, hat) and torch.equal(kw_sel, sel)
            # 1: the list does not change
            assert torch.equal(cm, p_cm) and torch.equal(ct, p_ct)
            cm_n, reg_n, sel_n, ok_n = cm.cpu().numpy(), reg.cpu().numpy(), sel.cpu().numpy(), ok.cpu().numpy()
            # 2: the remainder of every candidate
            assert reg.dtype == torch.int32 and np.array_equal(reg_n, C.cand_remainders(cm_n, poly))
            unused = (cm_n == 0).all(2)
            assert unused.sum() == B * max(0, L - 2 ** K) and (reg_n[unused] == -1).all()
            # 3
            assert np.array_equal(ok_n == 1, (reg_n == 0).any(1)) and set(np.unique(ok_n)) <= {0, 1}
            # 4: eligibility, and the float64 first minimum over the eligible candidates
            elig = np.where((reg_n == 0).any(1)[:, None], reg_n == 0, reg_n >= 0)
            assert elig[rows, sel_n].all()
            cwd = encode(code, cm.reshape(B * L, K)).reshape(B, L, N).double()
            dist = ((cwd - y.double()[:, None, :]) ** 2).sum(2).cpu().numpy()
            de = np.where(elig, dist, np.inf)
            clear = C.eligible_gap(cm_n, dist, poly) >= H.DIST_MARGIN
            assert np.array_equal(sel_n[clear], de.argmin(1)[clear])
            assert (dist[rows, sel_n] - de.min(1) <= H.DIST_MARGIN).all()
            r_sel, r_ok, _ = C.ca_choice(cm_n, dist, poly)
            assert np.array_equal(r_ok, ok_n) and np.array_equal(r_sel[clear], sel_n[clear])
            # 5: against the plain decoder
            none = ok_n == 0
            ps = p_sel.cpu().numpy()
            assert np.array_equal(sel_n[none], ps[none]) and torch.equal(p_hat[torch.from_numpy(none).to(DEV)][:, :K - c],
                                                                         hat[torch.from_numpy(none).to(DEV)])
            plain_ok = reg_n[rows, ps] == 0
            assert np.array_equal(sel_n[plain_ok], ps[plain_ok])
            # 6
            assert hat.shape == (B, K - c)
            assert torch.equal(hat, cm[torch.arange(B, device=DEV), sel.long()][:, :K - c])
            out = {"reg": reg_n, "sel": sel_n, "ok": ok_n, "plain_sel": ps, "dist": dist, "cm": cm_n}
        return out
    finally:
        code.set_crc(0)


# ------------------------------------------------------------------------------------------------ seeded nets
@pytest.mark.parametrize("L", LISTS)
@pytest.mark.parametrize("poly", [0xB, 0x3], ids=["crc3", "crc1"])
def test_polar_32_16_one_bit_word(poly, L):
    """Polar(32,16), F = 64 x 1, no onehot: one bit word, Lp = 1 / 2 / 4 / 8.  With polynomial 0xB the kernel's own
    outputs at B = 515 meet the input conditions: every class of the rule holds >= 5 % of the words."""
    out = check_invariants("polar_32_16_f64_l1", poly, L, BATCHES)
    if poly == 0xB and L > 1:
        none, plain, other = C.classes(out["reg"], out["plain_sel"])
        print(f"L = {L}: no path passes {none:.3f}, plain choice passes {plain:.3f}, another path passes {other:.3f}")
        assert min(none, plain, other) >= 0.05
        assert C.eligible_gap(out["cm"], out["dist"], poly).min() >= H.DIST_MARGIN


@pytest.mark.parametrize("L", LISTS)
@pytest.mark.parametrize("poly", [0x1D5, 0x11021, 0x1B2B117], ids=["crc8", "crc16", "crc24"])
def test_polar_64_32_two_bit_words_long_registers(poly, L):
    """Polar(64,32), F = 64 x 2: two bit words and registers of 8, 16 and 24 bits.  Hardly any path passes, which is why
    the remainder itself is an output: it checks the long division on every candidate."""
    check_invariants("polar_64_32_f64_l2", poly, L, BATCHES)


@pytest.mark.parametrize("L", LISTS)
def test_pac_32_10_crc_covers_v(L):
    """PAC(32,10), g = 53, F = 32 x 2: the CRC is on the path's v bits (the message before the convolution), the
    distance on the convolved and transformed word."""
    check_invariants("pac_32_10_f32_l2", 0xB, L, BATCHES)


def test_polar_256_128_all_eight_bit_words():
    check_invariants("polar_256_128_f32_l1", 0x1D5, 4, [33])


@pytest.mark.parametrize("L", [3, 4, 8])
def test_unused_slots_carry_minus_one(L):
    """Polar(8,2): four messages, so a list of 8 has four unused slots (remainder -1, never eligible)."""
    out = check_invariants("polar_8_2_f32_l1", 0x3, L, [7, 33])
    assert (out["reg"][:, 4:] == -1).all() and (out["reg"][:, :min(L, 4)] >= 0).all() and (out["sel"] < 4).all()


@pytest.mark.parametrize("L", [2, 8])
def test_wide_kernel(L):
    """gru_wide_list_kernel (F = 256, weights streamed): Polar(16,8), B in {7, 33}."""
    check_invariants("polar_16_8_f256_l1", 0xB, L, [7, 33])


# ------------------------------------------------------------------------------------------------ trained net
@functools.lru_cache(maxsize=None)
def trained():
    """(fixture, code, info, net, decoder) of the trained Polar(32,16) net; built once and left unchanged."""
    from neural_polar_decoder_amd.rnn import RNN_decoder, RNN_Model
    d, sd = H.load_fixture("rnnl_polar_32_16")
    N, K = int(d["N"]), int(d["K"])
    code, info = code_of(N, K)
    assert np.array_equal(info, d["info"])
    net = RNN_Model("GRU", N + 1 + int(d["onehot"]), int(d["F"]), 1, int(d["layers"]), N, 0, 0).to(DEV).eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return d, sd, code, info, net, RNN_decoder("y_input", N, info, onehot=bool(d["onehot"]))


@functools.lru_cache(maxsize=None)
def trained_words(poly):
    d, _, _, info, _, _ = trained()
    return C.ca_words(int(d["N"]), int(d["K"]), info, 2, poly, snr=1.0, B=512, seed=7)


@pytest.mark.parametrize("L", [2, 4, 8])
@pytest.mark.parametrize("poly", [0xB, 0x1D5], ids=["crc3", "crc8"])
def test_trained_net_matches_the_float64_restatement(poly, L):
    """Words that carry a CRC, at 1 dB, against list_decode_np + ca_choice.  Robust words (every prune margin
    >= 2 K LOGIT_ATOL, eligible-distance gap >= DIST_MARGIN): msg_hat, crc_ok and the candidate set identical, none
    exempt; over all words >= 99 % of msg_hat rows identical; robust share >= 0.70."""
    d, sd, code, info, net, dec = trained()
    N, K = int(d["N"]), int(d["K"])
    c = crc_degree(poly)
    _, _, _, y = trained_words(poly)
    ref = C.ca_list_decode_np(sd, N, info, int(d["onehot"]), int(d["layers"]), y, L, poly)
    code.set_crc(c, poly)
    try:
        hat, ok, (cm, ct, sel, reg) = dec.list_decode_crc(net, torch.from_numpy(y).to(DEV), code, L, return_ok=True,
                                                          return_candidates=True)
    finally:
        code.set_crc(0)
    hat, ok, cm, ct = hat.cpu().numpy(), ok.cpu().numpy(), cm.cpu().numpy(), ct.cpu().numpy()
    robust = (ref["prune_margin"] >= 2 * K * H.LOGIT_ATOL) & (ref["elig_gap"] >= H.DIST_MARGIN)
    same = (hat == ref["msg"][:, :K - c]).all(1)
    gm, _ = H.sorted_candidates(cm, ct)
    rm, _ = H.sorted_candidates(ref["cand_msg"].astype(np.float32), ref["cand_metric"].astype(np.float32))
    same_set = (gm == rm).all((1, 2))
    print(f"poly {poly:#x} L = {L}: robust {robust.mean():.4f}, msg_hat identical {same.mean():.4f} (robust "
          f"{same[robust].mean():.4f}), candidate sets identical {same_set.mean():.4f}, crc_ok identical "
          f"{(ok == ref['crc_ok']).mean():.4f}, crc_ok share {ok.mean():.3f}")
    assert robust.mean() >= 0.70
    assert same[robust].all(), np.flatnonzero(robust & ~same)[:8]
    assert (ok == ref["crc_ok"])[robust].all(), np.flatnonzero(robust & (ok != ref["crc_ok"]))[:8]
    assert same_set[robust].all(), np.flatnonzero(robust & ~same_set)[:8]
    assert same.mean() >= 0.99, same.mean()


# ------------------------------------------------------------------------------------------------ counting
def expected_counts(dec, net, code, y, msg, L, kc):
    """[bit errors, block errors, words no path passed for] of list_decode_crc + count_errors over the first kc columns."""
    from neural_polar_decoder_amd.utils import count_errors
    hat, ok = dec.list_decode_crc(net, y, code, L, return_ok=True)
    two = count_errors(msg[:, :kc].contiguous(), hat.contiguous())
    return two.cpu().tolist() + [int((ok == 0).sum())]


@pytest.mark.parametrize("L", [1, 4, 8])
def test_fused_counters_equal_decode_then_count(L):
    """2^12 words that carry a CRC on the trained net, two codeword offsets: count for count."""
    d, _, code, info, net, dec = trained()
    K, B = int(d["K"]), 1 << 12
    code.set_crc(8)
    try:
        total = torch.zeros(3, dtype=torch.int64, device=DEV)
        want = [0, 0, 0]
        for off in (0, 77777):
            msg, _, y = code.mc_generate_crc(B, 1.0, seed=21, cw_offset=off, device=DEV)
            cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
            hat = torch.empty(B, K, device=DEV)
            dec.list_decode_crc_mc(net, y, code, L, 21, off, cnt, msg_hat=hat)
            exp = expected_counts(dec, net, code, y, msg, L, K - 8)
            assert cnt.cpu().tolist() == exp, (off, cnt.cpu().tolist(), exp)
            assert torch.equal(hat[:, :K - 8], dec.list_decode_crc(net, y, code, L))
            assert exp[1] > 0 and exp[2] > 0  # the words do produce errors and CRC failures
            dec.list_decode_crc_mc(net, y, code, L, 21, off, total)  # accumulates, no reset
            want = [a + b for a, b in zip(want, exp)]
        assert total.cpu().tolist() == want
    finally:
        code.set_crc(0)


@pytest.mark.parametrize("L", [1, 4, 8])
def test_polynomial_zero_counts_the_plain_choice_over_all_k_bits(L):
    from neural_polar_decoder_amd.utils import count_errors
    d, _, code, info, net, dec = trained()
    B = 1 << 12
    assert code.CRC_len == 0
    msg, _, y = code.mc_generate(B, 1.0, seed=22, cw_offset=5, device=DEV)
    cnt = torch.tensor([0, 0, 77], dtype=torch.int64, device=DEV)
    dec.list_decode_crc_mc(net, y, code, L, 22, 5, cnt)
    exp = count_errors(msg, dec.list_decode(net, y, code, L)).cpu().tolist()
    assert cnt.cpu().tolist() == exp + [77] and exp[1] > 0


@pytest.mark.parametrize("name,poly,L", [("polar_256_200_f32_l1", 0xE21, 4), ("polar_256_200_f32_l1", 0, 2),
                                         ("polar_256_128_f32_l1", 0x1D5, 4), ("polar_16_8_f256_l1", 0xB, 8),
                                         ("pac_32_10_f32_l2", 0xB, 3)],
                         ids=["k200_second_philox_block", "k200_no_crc", "k128", "wide", "pac"])
def test_fused_counters_at_the_other_shapes(name, poly, L):
    """K = 200 needs the second Philox block of message words (K - c > 128); the wide kernel and a PAC code count alike."""
    from neural_polar_decoder_amd.utils import count_errors
    code, info, net, dec, _ = shape_setup(name)
    K, B = SHAPES[name][1], 33
    cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
    if poly == 0:
        msg, _, y = code.mc_generate(B, 2.0, seed=23, cw_offset=9, device=DEV)
        dec.list_decode_crc_mc(net, y, code, L, 23, 9, cnt)
        exp = count_errors(msg, dec.list_decode(net, y, code, L)).cpu().tolist() + [0]
    else:
        c = crc_degree(poly)
        code.set_crc(c, poly)
        try:
            msg, _, y = code.mc_generate_crc(B, 2.0, seed=23, cw_offset=9, device=DEV)
            dec.list_decode_crc_mc(net, y, code, L, 23, 9, cnt)
            exp = expected_counts(dec, net, code, y, msg, L, K - c)
        finally:
            code.set_crc(0)
    assert cnt.cpu().tolist() == exp and exp[0] > 0, (cnt.cpu().tolist(), exp)


def test_monte_carlo_driver_batches_add_up():
    from neural_polar_decoder_amd.montecarlo import CAGRUListMonteCarlo
    d, _, code, info, net, dec = trained()
    code.set_crc(3)
    try:
        snrs, n = [0.0, 2.0], 2048
        one = CAGRUListMonteCarlo(code, net, dec, 4, snrs, n, n, seed=31, device=DEV)
        r1 = one.run()
        two = CAGRUListMonteCarlo(code, net, dec, 4, snrs, n, n // 2, seed=31, device=DEV)
        r2 = two.run()
        assert one.K == int(d["K"]) - 3 and r1.K == one.K and one.crc_len == 3
        assert list(r1.bit_errors) == list(r2.bit_errors) and list(r1.block_errors) == list(r2.block_errors)
        assert one.crc_fail == two.crc_fail and len(one.crc_fail) == 2 and one.crc_fail[0] > 0
        assert r1.block_errors[0] > r1.block_errors[1] > 0
        # the first point once more by hand
        msg, _, y = code.mc_generate_crc(n, snrs[0], 31, 0, 0, device=DEV)
        exp = expected_counts(dec, net, code, y, msg, 4, one.K)
        assert [int(r1.bit_errors[0]), int(r1.block_errors[0]), one.crc_fail[0]] == exp
    finally:
        code.set_crc(0)


# ------------------------------------------------------------------------------------------------ the rest
def test_graph_capture_and_replay_equal_eager():
    """Both entry points on one captured stream (no parallel branches)."""
    code, info, net, dec, y_all = shape_setup("polar_64_32_f64_l2")
    code.set_crc(8)
    try:
        y = y_all[:33].clone()
        eager = dec.list_decode_crc(net, y, code, 4, return_ok=True, return_candidates=True)
        ecnt = torch.zeros(3, dtype=torch.int64, device=DEV)
        dec.list_decode_crc_mc(net, y, code, 4, 3, 0, ecnt)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):  # warm-up on the side stream: handle built, attribute set
            dec.list_decode_crc(net, y, code, 4)
            dec.list_decode_crc_mc(net, y, code, 4, 3, 0, torch.zeros(3, dtype=torch.int64, device=DEV))
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = dec.list_decode_crc(net, y, code, 4, return_ok=True, return_candidates=True)
            dec.list_decode_crc_mc(net, y, code, 4, 3, 0, cnt)
        flat = (out[0], out[1]) + tuple(out[2])
        for t in flat + (cnt,):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(flat, (eager[0], eager[1]) + tuple(eager[2])):
            assert torch.equal(a, b)
        assert torch.equal(cnt, ecnt)
    finally:
        code.set_crc(0)


def test_empty_batch_and_optional_outputs():
    from neural_polar_decoder_amd import _lib
    code, info, net, dec, y_all = shape_setup("polar_32_16_f64_l1")
    N, K, Ls, poly = 32, 16, 4, 0xB
    code.set_crc(3)
    try:
        hat, ok, (cm, ct, sel, reg) = dec.list_decode_crc(net, y_all[:0], code, Ls, return_ok=True, return_candidates=True)
        assert hat.shape == (0, K - 3) and ok.shape == (0,) and cm.shape == (0, Ls, K) and reg.shape == (0, Ls)
        cnt = torch.tensor([1, 2, 3], dtype=torch.int64, device=DEV)
        dec.list_decode_crc_mc(net, y_all[:0], code, Ls, 1, 0, cnt)
        assert cnt.cpu().tolist() == [1, 2, 3]
        B = 33
        y = y_all[:B].contiguous()
        f_hat, f_ok, (f_cm, f_ct, f_sel, f_reg) = dec.list_decode_crc(net, y, code, Ls, return_ok=True,
                                                                       return_candidates=True)
        lib, h, ch = _lib.load(), dec._handle(net, y.device), code.code
        s = _lib.stream_of(y.device)
        p = _lib.ptr
        fn, mc = lib.npd_gru_list_decode_crc, lib.npd_gru_list_decode_crc_mc
        # B = 0 with NULL operands: NPD_OK, nothing launched
        assert fn(h.h, ch.h, None, None, Ls, poly, None, None, None, None, None, None, 0, s) == 0
        assert mc(h.h, ch.h, None, None, Ls, poly, None, 1, 0, 0, p(cnt), s) == 0
        # msg_hat alone (all K columns, the CRC's included)
        hat2 = torch.full((B, K), 7.0, device=DEV)
        assert fn(h.h, ch.h, p(y), None, Ls, poly, p(hat2), None, None, None, None, None, B, s) == 0
        assert torch.equal(hat2, f_cm[torch.arange(B, device=DEV), f_sel.long()]) and torch.equal(hat2[:, :K - 3], f_hat)
        # msg_hat with crc_ok; msg_hat with sel
        ok2 = torch.full((B,), 7, dtype=torch.int32, device=DEV)
        sel2 = torch.full((B,), 7, dtype=torch.int32, device=DEV)
        assert fn(h.h, ch.h, p(y), None, Ls, poly, p(hat2), None, p(ok2), None, None, None, B, s) == 0
        assert torch.equal(ok2, f_ok) and torch.all(sel2 == 7)
        assert fn(h.h, ch.h, p(y), p(y), Ls, poly, p(hat2), p(sel2), None, None, None, None, B, s) == 0
        assert torch.equal(sel2, f_sel)
        # candidates alone, then with their metrics and remainders one at a time
        cm2, ct2 = torch.full((B, Ls, K), 7.0, device=DEV), torch.full((B, Ls), 7.0, device=DEV)
        reg2 = torch.full((B, Ls), 7, dtype=torch.int32, device=DEV)
        assert fn(h.h, ch.h, p(y), None, Ls, poly, None, None, None, p(cm2), None, None, B, s) == 0
        assert torch.equal(cm2, f_cm) and torch.all(ct2 == 7) and torch.all(reg2 == 7)
        assert fn(h.h, ch.h, p(y), None, Ls, poly, None, None, None, p(cm2), p(ct2), None, B, s) == 0
        assert torch.equal(ct2, f_ct) and torch.all(reg2 == 7)
        assert fn(h.h, ch.h, p(y), None, Ls, poly, None, None, None, p(cm2), None, p(reg2), B, s) == 0
        assert torch.equal(reg2, f_reg)
        # the counting entry point without and with msg_hat
        c1 = torch.zeros(3, dtype=torch.int64, device=DEV)
        c2 = torch.zeros(3, dtype=torch.int64, device=DEV)
        hat3 = torch.full((B, K), 7.0, device=DEV)
        assert mc(h.h, ch.h, p(y), None, Ls, poly, None, 1, 0, B, p(c1), s) == 0
        assert mc(h.h, ch.h, p(y), None, Ls, poly, p(hat3), 1, 0, B, p(c2), s) == 0
        assert torch.equal(c1, c2) and torch.equal(hat3, hat2) and int(c1[2]) == int((f_ok == 0).sum())
        # neither msg_hat nor cand_msg; NULL y; polynomial 0; bad list size; another code length; misaligned y
        assert fn(h.h, ch.h, p(y), None, Ls, poly, None, p(sel2), p(ok2), None, p(ct2), p(reg2), B, s) == -1
        assert fn(h.h, ch.h, None, None, Ls, poly, p(hat2), None, None, None, None, None, B, s) == -1
        assert fn(h.h, ch.h, p(y), None, Ls, 0, p(hat2), None, None, None, None, None, B, s) == -1
        assert fn(h.h, ch.h, p(y), None, 9, poly, p(hat2), None, None, None, None, None, B, s) == -1
        assert mc(h.h, ch.h, None, None, Ls, poly, None, 1, 0, B, p(c1), s) == -1
        assert mc(h.h, ch.h, p(y), None, Ls, poly, None, 1, 0, B, None, s) == -1
        other = code_of(16, 8)[0].code
        assert fn(h.h, other.h, p(y), None, Ls, poly, p(hat2), None, None, None, None, None, B, s) == -1
        assert fn(h.h, ch.h, y.data_ptr() + 4, None, Ls, poly, p(hat2), None, None, None, None, None, B, s) == -1
        torch.cuda.synchronize()
    finally:
        code.set_crc(0)


def test_unsupported_handles_return_enotsup():
    from neural_polar_decoder_amd import _lib
    from neural_polar_decoder_amd.rnn import RNN_decoder, RNN_Model
    code, info = code_of(16, 8)
    code.set_crc(3)
    N, K = 16, 8
    y = torch.zeros(4, N, device=DEV)
    hat = torch.zeros(4, K, device=DEV)
    cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    nets = [(RNN_Model("LSTM", N + 2, 32, 1, 1, N, 0, 0), "fp32"), (RNN_Model("GRU", N + 2, 128, 1, 1, N, 0, 0), "fp32"),
            (RNN_Model("GRU", N + 2, 32, 1, 2, N, 0, 0), "fp16x3")]
    for net, precision in nets:
        net = net.to(DEV).eval()
        dec = RNN_decoder("y_input", N, info, onehot=True, precision=precision)
        with pytest.raises(_lib.NpdError):
            dec.list_decode_crc(net, y, code, 4)
        h = dec._handle(net, y.device)
        s = _lib.stream_of(y.device)
        assert lib.npd_gru_list_decode_crc(h.h, code.code.h, _lib.ptr(y), None, 4, 0xB, _lib.ptr(hat), None, None, None,
                                           None, None, 4, s) == -2
        assert lib.npd_gru_list_decode_crc_mc(h.h, code.code.h, _lib.ptr(y), None, 4, 0xB, None, 1, 0, 4, _lib.ptr(cnt),
                                              s) == -2
    torch.cuda.synchronize()


def test_use_ynn_feeds_fy_to_the_counting_launch():
    """--use_ynn: the GRU sees Fy = get_Fy(y), the selection the raw y -- list_decode_crc_mc against list_decode_crc."""
    from conftest import golden
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.rnn import RNN_decoder, RNN_Model
    d = golden("gru_ynn_polar_16_8_d1_noonehot.npz")
    N, F, layers, K = int(d["N"]), int(d["F"]), int(d["layers"]), len(d["info"])
    net = RNN_Model("GRU", N + 1 + int(d["onehot"]), F, 1, layers, N, int(d["y_hidden"]), int(d["y_depth"]),
                    bytes(d["activation"]).decode(), 0.0, False, y_output_size=N).to(DEV).eval()
    net.load_state_dict({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w.")})
    code = reference_polar_code(N, K)
    info = np.sort(np.asarray(code.info_positions))
    dec = RNN_decoder("y_input", N, info, onehot=bool(d["onehot"]))
    code.set_crc(3)
    msg, _, y = code.mc_generate_crc(515, 1.0, seed=41, cw_offset=3, device=DEV)
    cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
    dec.list_decode_crc_mc(net, y, code, 4, 41, 3, cnt)
    assert cnt.cpu().tolist() == expected_counts(dec, net, code, y, msg, 4, K - 3)
    hat, (cm, _, sel, _) = dec.list_decode_crc(net, y, code, 4, return_candidates=True)
    _, (p_cm, _, _) = dec.list_decode(net, y, code, 4, return_candidates=True)
    assert torch.equal(cm, p_cm) and torch.equal(hat, cm[torch.arange(515, device=DEV), sel.long()][:, :K - 3])
