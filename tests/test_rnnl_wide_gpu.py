"""GRU list decoding at hidden 256 / 512 on the MI355X (gru_wide_list_kernel behind npd_gru_list_decode).

Against the reference's recorded runs (tests/golden/gen_rnnl_wide.py), at each fixture's tolerance
(rnnl_wide_helper.LOGIT_TOL = max(2e-5, 2 E), E measured on the greedy wide kernel):
  * every ROBUST word of the three seeded fixtures has the reference's msg_hat and candidate set, in list order;
    >= 99 % of all msg_hat rows are the reference's; metrics within K tol on identical sets;
  * the trained hidden-512 x 2 Polar(64,22) net: msg_L4 equal on >= 99 % of 256 words, and the L = 4 Monte-Carlo curve
    at 0, 1, 2 dB within 4 sigma (BER and BLER) of the reference's recorded counts.
Invariants on seeded nets, (N 16, F 256, 1 layer) and (N 32, F 512, 2 layers), B in {1, 5, 33, 70} (a tile holds 32, 16,
8 or 4 words, so the ragged tail differs for every padded list size):
  1. L = 1 is the greedy decoder (gru_wide_kernel), bit for bit, every metric 0 and sel 0;
  2. with no pruning (2^K <= L) the answer is ML wherever the ML gap exceeds its bound;
  3. metrics are teacher-forced logit sums (fp32, step order), within 2e-5 per flipped position;
  4. sel is the first minimum of ||encode(cand) - y||^2 wherever the two smallest differ by >= 1e-3;
  5. no message repeats within a list.
Plus exact metric ties (torch.topk's rule), --use_ynn, graph capture, B = 0 and the optional outputs.
"""
import argparse

import numpy as np
import pytest
import torch

import rnnl_wide_helper as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = [1, 5, 33, 70]


def net_of(sd, N, F, layers, onehot):
    from neural_polar_decoder_amd.rnn import RNN_Model
    net = RNN_Model("GRU", N + 1 + int(onehot), F, 1, layers, N, 0, 0).to(DEV).eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net


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


def full_words(cand, info, N):
    """(M, K) candidates -> (M, N) words with +1 at the frozen positions."""
    w = torch.ones(cand.shape[0], N, device=cand.device)
    w[:, torch.as_tensor(info, device=cand.device)] = cand
    return w


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", list(W.SEEDED))
def test_fixture_words_match_the_reference(name):
    from neural_polar_decoder_amd.rnn import RNN_decoder
    d, sd = W.load_fixture(name)
    N, K, tol = int(d["N"]), int(d["K"]), W.LOGIT_TOL[name]
    code, info = code_of(N, K, int(d["g"]) if int(d["pac"]) else 0)
    assert np.array_equal(info, d["info"])
    net = net_of(sd, N, int(d["F"]), int(d["layers"]), int(d["onehot"]))
    dec = RNN_decoder("y_input", N, info, onehot=bool(d["onehot"]))
    y = torch.from_numpy(d["y"]).to(DEV)
    for L in W.SEEDED[name][1]:
        hat, (cm, ct, sel) = dec.list_decode(net, y, code, L, return_candidates=True)
        hat, cm, ct = hat.cpu().numpy(), cm.cpu().numpy(), ct.cpu().numpy()
        ref = W.unpack_pm1(d[f"msg_L{L}"], K)
        rcm, rct = W.unpack_pm1(d[f"cand_L{L}"], K), d[f"cand_metric_L{L}"]
        robust = W.robust_mask(d, L, tol)
        same = (hat == ref).all(1)
        gm, gt = W.sorted_candidates(cm, ct)
        rm, rt = W.sorted_candidates(rcm, rct)
        same_set = (gm == rm).all((1, 2))
        err = np.abs(gt[same_set] - rt[same_set]).max()
        print(f"{name} L = {L}: msg_hat identical {same.mean():.4f} (robust words {robust.mean():.4f}: "
              f"{same[robust].mean():.4f}), candidate sets identical {same_set.mean():.4f} "
              f"(robust: {same_set[robust].mean():.4f}), metric error {err:.3e}")
        assert d[f"stable_L{L}"].mean() >= W.STABLE_MIN
        assert robust.mean() >= W.ROBUST_MIN
        assert same[robust].all(), (L, np.flatnonzero(robust & ~same)[:8])
        assert same_set[robust].all(), (L, np.flatnonzero(robust & ~same_set)[:8])
        assert same.mean() >= 0.99, (L, same.mean())
        assert err <= K * tol, (L, err)
        # list order too, where the set is the reference's: ascending child index is part of the contract
        assert (cm[same_set & robust] == rcm[same_set & robust]).all()


_trained = {}


def trained_setup():
    """(fixture, code, info, net, decoder) of the trained hidden-512 x 2 Polar(64,22) net, built once."""
    if not _trained:
        from neural_polar_decoder_amd.rnn import RNN_decoder
        d, sd = W.load_fixture(W.TRAINED)
        N, K = int(d["N"]), int(d["K"])
        code, info = code_of(N, K)
        assert np.array_equal(info, d["info"])
        net = net_of(sd, N, int(d["F"]), int(d["layers"]), int(d["onehot"]))
        _trained["x"] = (d, code, info, net, RNN_decoder("y_input", N, info, onehot=bool(d["onehot"])))
    return _trained["x"]


def test_trained_net_words_match_the_reference():
    """The net's outputs saturate near +-1, so metrics with equal flip counts nearly tie and few words are robust
    (0.41 at L = 4): there is no word-exact bar beyond the global one."""
    d, code, info, net, dec = trained_setup()
    K = int(d["K"])
    hat = dec.list_decode(net, torch.from_numpy(d["y"]).to(DEV), code, 4).cpu().numpy()
    same = (hat == W.unpack_pm1(d["msg_L4"], K)).all(1)
    robust = W.robust_mask(d, 4, W.LOGIT_ATOL)
    print(f"{W.TRAINED} L = 4: msg_hat identical {same.mean():.4f} (robust words {robust.mean():.4f}: "
          f"{same[robust].mean():.4f})")
    assert same.mean() >= 0.99, same.mean()


def test_trained_net_curve_matches_the_reference():
    from neural_polar_decoder_amd.montecarlo import GRUListMonteCarlo
    d, code, info, net, dec = trained_setup()
    L = int(d["curve_L"])
    snrs = [float(s) for s in d["curve_snr"]]
    n, nr = 1 << 15, int(d["curve_n"])
    mc = GRUListMonteCarlo(code, net, dec, L, snrs, n, n, seed=2041)
    res = mc.run()
    for si, s in enumerate(snrs):
        # the same words decoded once more for the per-word error counts (the BER variance)
        msg, y = mc.generate(si, s, 0, n)
        e = (dec.list_decode(net, y, code, L) != msg).sum(1).to(torch.int64)
        be, bl, sq = int(e.sum()), int((e > 0).sum()), int((e * e).sum())
        assert be == int(res.bit_errors[si]) and bl == int(res.block_errors[si])
        rbe, rbl, rsq = int(d["curve_bit_err"][si]), int(d["curve_blk_err"][si]), int(d["curve_sq_err"][si])
        p, pr = bl / n, rbl / nr
        pool = (bl + rbl) / (n + nr)
        z_bler = (p - pr) / np.sqrt(pool * (1 - pool) * (1 / n + 1 / nr))
        v, vr = sq / n - (be / n) ** 2, rsq / nr - (rbe / nr) ** 2
        z_ber = (be / n - rbe / nr) / np.sqrt(v / n + vr / nr)
        print(f"{s} dB L = {L}: BLER {p:.4e} (reference {pr:.4e}, z {z_bler:.2f}), BER z {z_ber:.2f}")
        assert abs(z_bler) < 4 and abs(z_ber) < 4, (s, p, pr, z_bler, z_ber)


# ------------------------------------------------------------------------------------------------ invariants
SHAPES = {  # name: (N, K, pac_g, F, layers, onehot)
    "polar_16_8_f256_l1": (16, 8, 0, 256, 1, False),
    "polar_32_16_f512_l2": (32, 16, 0, 512, 2, True),
}
_cache = {}


def shape_setup(name):
    """(code, info, net, decoder, y (70, N) on the device), built once per shape and left unchanged."""
    if name not in _cache:
        from neural_polar_decoder_amd.montecarlo import seeded_crisp
        N, K, g, F, layers, onehot = SHAPES[name]
        code, info = code_of(N, K, g)
        net, dec = seeded_crisp(code, F, layers, seed=11, device=DEV, onehot=onehot)
        with torch.no_grad():  # PyTorch-default weights give logits ~0.1: scale so that paths separate
            for k, p in net.named_parameters():
                p.mul_(3.0 if k.startswith("rnn.") else 10.0)
        gen = torch.Generator().manual_seed(5)
        msg = 1.0 - 2.0 * (torch.rand(max(BATCHES), K, generator=gen) < 0.5).float()
        y = encode(code, msg.to(DEV)) + 0.7 * torch.randn(max(BATCHES), N, generator=gen).to(DEV)
        _cache[name] = (code, info, net, dec, y)
    return _cache[name]


# the longest length the interface takes (N = 256: 256 steps, every word of the path-bit masks in use), K = 128; the
# exact invariants only -- the tolerance-based ones stay at the shapes above
LONG_SHAPE = (256, 128, 0, 256, 1, False)


def long_setup():
    """shape_setup's recipe at LONG_SHAPE, 33 words; built once and left unchanged."""
    if "long" not in _cache:
        from neural_polar_decoder_amd.montecarlo import seeded_crisp
        N, K, g, F, layers, onehot = LONG_SHAPE
        code, info = code_of(N, K, g)
        net, dec = seeded_crisp(code, F, layers, seed=11, device=DEV, onehot=onehot)
        with torch.no_grad():
            for k, p in net.named_parameters():
                p.mul_(3.0 if k.startswith("rnn.") else 10.0)
        gen = torch.Generator().manual_seed(5)
        msg = 1.0 - 2.0 * (torch.rand(33, K, generator=gen) < 0.5).float()
        y = encode(code, msg.to(DEV)) + 0.7 * torch.randn(33, N, generator=gen).to(DEV)
        _cache["long"] = (code, info, net, dec, y)
    return _cache["long"]


@pytest.mark.parametrize("L", [1, 4, 8])
@pytest.mark.parametrize("B", [1, 33])
def test_longest_length_exact_invariants(B, L):
    """N = 256, K = 128 on gru_wide_list_kernel.  Invariant 1: L = 1 is the greedy decoder bit for bit, every metric 0 and sel 0;
    invariant 5: no message repeats within a list (and every survivor is a +-1 word with a finite metric, msg_hat the
    selected one)."""
    code, info, net, dec, y_all = long_setup()
    y = y_all[:B]
    hat, (cm, ct, sel) = dec.list_decode(net, y, code, L, return_candidates=True)
    assert cm.shape == (B, L, LONG_SHAPE[1]) and torch.isfinite(ct).all() and (cm.abs() == 1).all()
    assert torch.equal(hat, cm[torch.arange(B, device=DEV), sel.long()])
    eq = (cm[:, :, None, :] == cm[:, None, :, :]).all(-1)
    assert int(eq.sum()) == B * L
    if L == 1:
        greedy = dec.decode(net, False, y)[:, torch.as_tensor(info, device=DEV)]
        assert torch.equal(hat, greedy)
        assert torch.equal(cm[:, 0], hat) and torch.all(ct == 0) and torch.all(sel == 0)
        if B > 1:  # over the batch the greedy decode is not a constant
            assert 0.05 < float((greedy < 0).float().mean()) < 0.95


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_list_size_one_is_the_greedy_decoder(name, B):
    code, info, net, dec, y = shape_setup(name)
    hat, (cm, ct, sel) = dec.list_decode(net, y[:B], code, 1, return_candidates=True)
    greedy = dec.decode(net, False, y[:B])[:, torch.as_tensor(info, device=DEV)]
    assert torch.equal(hat, greedy)
    assert torch.equal(cm[:, 0], hat) and torch.all(ct == 0) and torch.all(sel == 0)


@pytest.mark.parametrize("L", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("name", list(SHAPES))
def test_metrics_selection_and_distinct_survivors(name, L):
    """Invariants 3, 4 and 5 at every batch size (the ragged tile differs per padded list size)."""
    code, info, net, dec, y_all = shape_setup(name)
    N, K = SHAPES[name][0], SHAPES[name][1]
    it = torch.as_tensor(info, device=DEV)
    for B in BATCHES:
        y = y_all[:B]
        hat, (cm, ct, sel) = dec.list_decode(net, y, code, L, return_candidates=True)
        assert torch.isfinite(ct).all() and (cm.abs() == 1).all()
        assert torch.equal(hat, cm[torch.arange(B, device=DEV), sel.long()])
        # 5: distinct messages
        eq = (cm[:, :, None, :] == cm[:, None, :, :]).all(-1)
        assert int(eq.sum()) == B * L
        # 3: teacher-forced logit sums
        words = full_words(cm.reshape(B * L, K), info, N)
        y_rep = y.repeat_interleave(L, 0)
        _, lg = dec.decode(net, False, y_rep, gt=words, loss_inds=[], return_logits=True)
        lg = lg[:, it].cpu().numpy()
        bits = cm.reshape(B * L, K).cpu().numpy()
        flip = np.sign(lg) != bits
        exp = np.zeros(B * L, np.float32)
        for k in range(K):  # fp32, in step order
            exp = exp + np.where(flip[:, k], np.abs(lg[:, k]), 0).astype(np.float32)
        got = ct.reshape(-1).cpu().numpy()
        assert np.all(np.abs(got - exp) <= 2e-5 * np.maximum(flip.sum(1), 1)), np.abs(got - exp).max()
        # 4: first minimum of the float64 distance
        cwd = encode(code, cm.reshape(B * L, K)).reshape(B, L, N).double()
        dist = ((cwd - y.double()[:, None, :]) ** 2).sum(2).cpu().numpy()
        ds = np.sort(dist, 1)
        clear = ds[:, 1] - ds[:, 0] >= W.DIST_MARGIN
        assert clear.mean() >= 0.9 or B < 33
        assert np.array_equal(sel.cpu().numpy()[clear], dist.argmin(1)[clear])


@pytest.mark.parametrize("case", [(8, 3, 0), (8, 3, 13)], ids=["polar_8_3", "pac_8_3"])
def test_no_pruning_is_maximum_likelihood(case):
    from neural_polar_decoder_amd.codes import all_message_bits
    from neural_polar_decoder_amd.montecarlo import seeded_crisp
    N, K, g = case
    code, info = code_of(N, K, g)
    net, dec = seeded_crisp(code, 256, 1, seed=3, device=DEV, onehot=True)
    gen = torch.Generator().manual_seed(17)
    B = 515
    msg = 1.0 - 2.0 * (torch.rand(B, K, generator=gen) < 0.5).float()
    y = encode(code, msg.to(DEV)) + 0.8 * torch.randn(B, N, generator=gen).to(DEV)
    hat, (cm, ct, sel) = dec.list_decode(net, y, code, 8, return_candidates=True)
    # every message survives, once
    amb = torch.from_numpy(all_message_bits(K)).to(DEV)
    hits = (cm[:, :, None, :] == amb[None, None, :, :]).all(-1).sum(1)
    assert torch.all(hits == 1)
    assert torch.isfinite(ct).all() and torch.all(sel < 8)
    # ML wherever the correlation gap exceeds npd_ml_decode's bound and the distance gap the selection's
    cb = encode(code, amb).double()
    corr = (y.double() @ cb.T).cpu().numpy()
    top2 = np.sort(corr, 1)[:, -2:]
    eps = 2.0 * N * 2.0 ** -24 * np.abs(y.double().cpu().numpy()).sum(1)
    clear = (top2[:, 1] - top2[:, 0] >= 4 * eps) & (2 * (top2[:, 1] - top2[:, 0]) >= W.DIST_MARGIN)
    assert clear.mean() > 0.9
    ml = code.ml_decode(y).cpu().numpy()
    assert np.array_equal(hat.cpu().numpy()[clear], ml[clear])


def test_unused_slots_are_empty():
    """2^K < L: the slots past the 2^K survivors carry metric +inf and message 0, as on the narrow kernel."""
    from neural_polar_decoder_amd.montecarlo import seeded_crisp
    code, info = code_of(8, 2)
    net, dec = seeded_crisp(code, 256, 2, seed=3, device=DEV, onehot=True)
    y = torch.randn(37, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    hat, (cm, ct, sel) = dec.list_decode(net, y, code, 8, return_candidates=True)
    assert torch.isfinite(ct[:, :4]).all() and (cm[:, :4].abs() == 1).all()
    assert torch.all(torch.isinf(ct[:, 4:]) & (ct[:, 4:] > 0)) and torch.all(cm[:, 4:] == 0)
    assert torch.all(sel < 4) and torch.equal(hat, cm[torch.arange(37, device=DEV), sel.long()])


@pytest.mark.parametrize("L", [2, 3, 5, 8])
def test_exact_metric_ties_follow_torch_topk(L):
    """A net whose output is the constant 0.5 (output weights 0, bias 0.5): every path's metric is 0.5 x its number of
    flips, so classes of equal metrics straddle the L-th place at almost every prune and the survivors are whatever
    torch.topk keeps (npd_nth.hpp, run by every wave alike).  The expected list is pruneLists itself on the CPU."""
    from neural_polar_decoder_amd.montecarlo import seeded_crisp
    N, K = 16, 8
    code, info = code_of(N, K)
    net, dec = seeded_crisp(code, 256, 1, seed=2, device=DEV, onehot=True)
    with torch.no_grad():
        net.linear.weight.zero_()
        net.linear.bias.fill_(0.5)
    met = torch.zeros(1, 1)
    msgs = torch.ones(1, 0)
    for _ in range(K):
        ls = met.shape[0]
        met = torch.vstack([met, met + 0.5])
        msgs = torch.vstack([torch.hstack([msgs, torch.ones(ls, 1)]), torch.hstack([msgs, -torch.ones(ls, 1)])])
        if 2 * ls > L:  # rnn_all.py:563-578
            keep = torch.sort(torch.topk(-1 * met, L, 0)[1], 0)[0][:, 0]
            met, msgs = met[keep], msgs[keep]
    B = 67
    y = torch.randn(B, N, generator=torch.Generator().manual_seed(1)).to(DEV)
    _, (cm, ct, _) = dec.list_decode(net, y, code, L, return_candidates=True)
    assert torch.equal(ct.cpu(), met[:, 0].expand(B, L))
    assert torch.equal(cm.cpu(), msgs.expand(B, L, K))


# ------------------------------------------------------------------------------------------------ the rest
def test_graph_capture_and_replay_equal_eager():
    code, info, net, dec, y_all = shape_setup("polar_32_16_f512_l2")
    y = y_all[:33].clone()
    eager = dec.list_decode(net, y, code, 4, return_candidates=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        dec.list_decode(net, y, code, 4)  # warm-up on the side stream: handle built, attribute set
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = dec.list_decode(net, y, code, 4, return_candidates=True)
    for t in (out[0],) + tuple(out[1]):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0])
    for a, b in zip(out[1], eager[1]):
        assert torch.equal(a, b)


def test_empty_batch_and_optional_outputs():
    from neural_polar_decoder_amd import _lib
    code, info, net, dec, y_all = shape_setup("polar_16_8_f256_l1")
    N, K, Ls = 16, 8, 4
    hat, (cm, ct, sel) = dec.list_decode(net, y_all[:0], code, Ls, return_candidates=True)
    assert hat.shape == (0, K) and cm.shape == (0, Ls, K) and ct.shape == (0, Ls) and sel.shape == (0,)
    B = 33
    y = y_all[:B].contiguous()
    full = dec.list_decode(net, y, code, Ls, return_candidates=True)
    lib, h, ch = _lib.load(), dec._handle(net, y.device), code.code
    s = _lib.stream_of(y.device)
    p = _lib.ptr
    # B = 0 with NULL operands: NPD_OK, nothing launched
    assert lib.npd_gru_list_decode(h.h, ch.h, None, None, Ls, None, None, None, None, 0, s) == 0
    # msg_hat alone; the other buffers stay as they were
    hat2 = torch.full((B, K), 7.0, device=DEV)
    assert lib.npd_gru_list_decode(h.h, ch.h, p(y), None, Ls, p(hat2), None, None, None, B, s) == 0
    assert torch.equal(hat2, full[0])
    # candidates alone (fy given explicitly as y)
    cm2, ct2 = torch.full((B, Ls, K), 7.0, device=DEV), torch.full((B, Ls), 7.0, device=DEV)
    sel2 = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    assert lib.npd_gru_list_decode(h.h, ch.h, p(y), p(y), Ls, None, None, p(cm2), p(ct2), B, s) == 0
    assert torch.equal(cm2, full[1][0]) and torch.equal(ct2, full[1][1]) and torch.all(sel2 == 7)
    assert lib.npd_gru_list_decode(h.h, ch.h, p(y), None, Ls, None, p(sel2), p(cm2), None, B, s) == 0
    assert torch.equal(sel2, full[1][2])
    # neither msg_hat nor cand_msg; NULL y; bad list sizes; another code length
    assert lib.npd_gru_list_decode(h.h, ch.h, p(y), None, Ls, None, p(sel2), None, p(ct2), B, s) == -1
    assert lib.npd_gru_list_decode(h.h, ch.h, None, None, Ls, p(hat2), None, None, None, B, s) == -1
    assert lib.npd_gru_list_decode(h.h, ch.h, p(y), None, 9, p(hat2), None, None, None, B, s) == -1
    other = code_of(32, 16)[0].code
    assert lib.npd_gru_list_decode(h.h, other.h, p(y), None, Ls, p(hat2), None, None, None, B, s) == -1
    assert lib.npd_gru_list_supported(h.h, ch.h, Ls) == 1 and lib.npd_gru_list_supported(h.h, other.h, Ls) == 0
    assert lib.npd_gru_list_supported(h.h, ch.h, 9) == 0
    torch.cuda.synchronize()


def test_use_ynn_feeds_fy_and_selects_on_y():
    """--use_ynn at hidden 256: the GRU sees Fy = get_Fy(y), the selection the raw y.  Invariants 3 and 4."""
    from neural_polar_decoder_amd.rnn import RNN_decoder, RNN_Model
    N, K, F, L, B = 16, 8, 256, 4, 70
    code, info = code_of(N, K)
    torch.manual_seed(23)
    net = RNN_Model("GRU", N + 2, F, 1, 2, N, 32, 1, "selu", 0.0, False, y_output_size=N).to(DEV).eval()
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.mul_(3.0 if k.startswith("rnn.") else 10.0 if k.startswith("linear.") else 1.0)
    dec = RNN_decoder("y_input", N, info, onehot=True)
    gen = torch.Generator().manual_seed(29)
    msg = 1.0 - 2.0 * (torch.rand(B, K, generator=gen) < 0.5).float()
    y = encode(code, msg.to(DEV)) + 0.7 * torch.randn(B, N, generator=gen).to(DEV)
    assert not torch.equal(net.get_Fy(y), y)
    hat, (cm, ct, sel) = dec.list_decode(net, y, code, L, return_candidates=True)
    assert torch.equal(hat, cm[torch.arange(B, device=DEV), sel.long()])
    it = torch.as_tensor(info, device=DEV)
    words = full_words(cm.reshape(B * L, K), info, N)
    _, lg = dec.decode(net, False, y.repeat_interleave(L, 0), gt=words, loss_inds=[], return_logits=True)
    lg = lg[:, it].cpu().numpy()
    bits = cm.reshape(B * L, K).cpu().numpy()
    flip = np.sign(lg) != bits
    exp = np.zeros(B * L, np.float32)
    for k in range(K):
        exp = exp + np.where(flip[:, k], np.abs(lg[:, k]), 0).astype(np.float32)
    assert np.all(np.abs(ct.reshape(-1).cpu().numpy() - exp) <= 2e-5 * np.maximum(flip.sum(1), 1))
    cwd = code.encode_plotkin(cm.reshape(B * L, K)).reshape(B, L, N).double()
    dist = ((cwd - y.double()[:, None, :]) ** 2).sum(2).cpu().numpy()
    ds = np.sort(dist, 1)
    clear = ds[:, 1] - ds[:, 0] >= W.DIST_MARGIN
    assert clear.mean() > 0.9
    assert np.array_equal(sel.cpu().numpy()[clear], dist.argmin(1)[clear])
