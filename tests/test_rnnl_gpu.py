"""GRU list decoding on the MI355X (npd_gru_list_decode, RNN_decoder.list_decode; reference rnn_all.py:563-664).

Against the reference's recorded runs (tests/golden/rnnl_*.npz, gen_rnnl.py):
  * every ROBUST word (rnnl_helper.robust_mask: every prune boundary >= 2 K 2e-5, final distance gap >= 1e-3) has the
    reference's msg_hat and the reference's candidate set -- none exempt;
  * over all words >= 99 % of msg_hat rows are the reference's (the project's codeword bar for the GRU);
  * on words whose candidate sets are identical, cand_metric is within K 2e-5.
Invariants on seeded nets (no fixture; N = 128 PAC, F = 32 x 2 layers, F = 64 x 1 layer; B in {1, 7, 33, 515} so the
ragged tile differs for every padded list size):
  1. L = 1 is the greedy decoder, bit for bit, and every metric is 0;
  2. with no pruning (2^K <= L) the answer is ML wherever the ML gap exceeds its bound, and unused slots are empty;
  3. metrics are teacher-forced logit sums: sum over information i of |logit_i| [sign(logit_i) != bit_i] (fp32, step
     order), within 2e-5 per flipped position, with the logits of the existing kernel's teacher-forced decode;
  4. sel is the first minimum of ||encode(cand) - y||^2 (float64, the package's encoder) wherever the two smallest
     differ by >= 1e-3, and msg_hat == cand_msg[b, sel[b]];
  5. no message repeats within a list.
Plus the Monte-Carlo curve against the reference's, graph capture, B = 0, optional outputs, --use_ynn, and refusals.
"""
import argparse

import numpy as np
import pytest
import torch

import rnnl_helper as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = [1, 7, 33, 515]
LISTS = [1, 2, 3, 4, 5, 8]


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


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", list(H.FIXTURES))
def test_fixture_words_match_the_reference(name):
    from neural_polar_decoder_amd.rnn import RNN_decoder
    d, sd = H.load_fixture(name)
    N, K = int(d["N"]), int(d["K"])
    code, info = code_of(N, K, int(d["g"]) if int(d["pac"]) else 0)
    assert np.array_equal(info, d["info"])
    net = net_of(sd, N, int(d["F"]), int(d["layers"]), int(d["onehot"]))
    dec = RNN_decoder("y_input", N, info, onehot=bool(d["onehot"]))
    y = torch.from_numpy(d["y"]).to(DEV)
    for L in H.FIXTURES[name][1]:
        hat, (cm, ct, sel) = dec.list_decode(net, y, code, L, return_candidates=True)
        hat, cm, ct = hat.cpu().numpy(), cm.cpu().numpy(), ct.cpu().numpy()
        ref = H.unpack_pm1(d[f"msg_L{L}"], K)
        rcm, rct = H.unpack_pm1(d[f"cand_L{L}"], K), d[f"cand_metric_L{L}"]
        robust = H.robust_mask(d, L)
        same = (hat == ref).all(1)
        gm, gt = H.sorted_candidates(cm, ct)
        rm, rt = H.sorted_candidates(rcm, rct)
        same_set = (gm == rm).all((1, 2))
        err = np.abs(gt[same_set] - rt[same_set]).max()
        print(f"{name} L = {L}: msg_hat identical {same.mean():.4f} (robust words {robust.mean():.4f}: "
              f"{same[robust].mean():.4f}), candidate sets identical {same_set.mean():.4f} "
              f"(robust: {same_set[robust].mean():.4f}), metric error {err:.3e}")
        assert robust.mean() >= 0.70
        assert same[robust].all(), (L, np.flatnonzero(robust & ~same)[:8])
        assert same_set[robust].all(), (L, np.flatnonzero(robust & ~same_set)[:8])
        assert same.mean() >= 0.99, (L, same.mean())
        assert err <= K * H.LOGIT_ATOL, (L, err)
        # list order too, where the set is the reference's: ascending child index is part of the contract
        assert (cm[same_set & robust] == rcm[same_set & robust]).all()


# ------------------------------------------------------------------------------------------------ invariants
SHAPES = {  # name: (N, K, pac_g, F, layers, onehot)
    "pac_128_64_f32_l2": (128, 64, 91, 32, 2, True),
    "polar_32_16_f64_l1": (32, 16, 0, 64, 1, False),
    "polar_64_32_f64_l2": (64, 32, 0, 64, 2, True),
}
_cache = {}


def shape_setup(name):
    """(code, info, net, decoder, y (515, N) on the device), built once per shape and left unchanged."""
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


def full_words(cand, info, N):
    """(M, K) candidates -> (M, N) words with +1 at the frozen positions."""
    w = torch.ones(cand.shape[0], N, device=cand.device)
    w[:, torch.as_tensor(info, device=cand.device)] = cand
    return w


# the longest length the interface takes (N = 256: 256 steps, every word of the path-bit masks in use), K = 128; the
# exact invariants only -- the tolerance-based ones stay at the shapes above
LONG_SHAPE = (256, 128, 0, 64, 2, True)


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
    """N = 256, K = 128 on gru_list_kernel.  Invariant 1: L = 1 is the greedy decoder bit for bit, every metric 0 and sel 0;
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


@pytest.mark.parametrize("L", LISTS)
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
        clear = np.ones(B, bool) if L == 1 else (ds[:, 1] - ds[:, 0] >= H.DIST_MARGIN)
        assert clear.mean() >= 0.9 or B < 33
        assert np.array_equal(sel.cpu().numpy()[clear], dist.argmin(1)[clear])


@pytest.mark.parametrize("case", [(8, 3, 0), (8, 2, 0), (8, 3, 13)], ids=["polar_8_3", "polar_8_2", "pac_8_3"])
def test_no_pruning_is_maximum_likelihood(case):
    from neural_polar_decoder_amd.codes import all_message_bits
    from neural_polar_decoder_amd.montecarlo import seeded_crisp
    N, K, g = case
    code, info = code_of(N, K, g)
    net, dec = seeded_crisp(code, 32, 1, seed=3, device=DEV, onehot=True)
    gen = torch.Generator().manual_seed(17)
    B = 515
    msg = 1.0 - 2.0 * (torch.rand(B, K, generator=gen) < 0.5).float()
    y = encode(code, msg.to(DEV)) + 0.8 * torch.randn(B, N, generator=gen).to(DEV)
    hat, (cm, ct, sel) = dec.list_decode(net, y, code, 8, return_candidates=True)
    n = min(8, 2 ** K)
    # every message survives, once; the slots past min(L, 2^K) are empty
    amb = torch.from_numpy(all_message_bits(K)).to(DEV)
    hits = (cm[:, :n, None, :] == amb[None, None, :, :]).all(-1).sum(1)
    assert torch.all(hits == 1)
    assert torch.isfinite(ct[:, :n]).all()
    assert torch.all(torch.isinf(ct[:, n:]) & (ct[:, n:] > 0)) and torch.all(cm[:, n:] == 0)
    assert torch.all(sel < n)
    # ML wherever the correlation gap exceeds npd_ml_decode's bound and the distance gap the selection's
    cb = encode(code, amb).double()
    corr = (y.double() @ cb.T).cpu().numpy()
    top2 = np.sort(corr, 1)[:, -2:]
    eps = 2.0 * N * 2.0 ** -24 * np.abs(y.double().cpu().numpy()).sum(1)
    clear = (top2[:, 1] - top2[:, 0] >= 4 * eps) & (2 * (top2[:, 1] - top2[:, 0]) >= H.DIST_MARGIN)
    assert clear.mean() > 0.9
    ml = code.ml_decode(y).cpu().numpy()
    assert np.array_equal(hat.cpu().numpy()[clear], ml[clear])


@pytest.mark.parametrize("L", [2, 3, 4, 5, 8])
def test_exact_metric_ties_follow_torch_topk(L):
    """A net whose output is the constant 0.5 (output weights 0, bias 0.5): every path's metric is 0.5 x its number of
    flips, so classes of equal metrics straddle the L-th place at almost every prune and the survivors are whatever
    torch.topk keeps (the kernel's npd_nth.hpp path).  The expected list is pruneLists itself on the CPU."""
    from neural_polar_decoder_amd.montecarlo import seeded_crisp
    N, K = 16, 8
    code, info = code_of(N, K)
    net, dec = seeded_crisp(code, 32, 1, seed=2, device=DEV, onehot=True)
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


# ------------------------------------------------------------------------------------------------ curve
def test_monte_carlo_curve_matches_the_reference_and_beats_greedy():
    from neural_polar_decoder_amd.montecarlo import GRUListMonteCarlo, GRUMonteCarlo
    from neural_polar_decoder_amd.rnn import RNN_decoder
    d, sd = H.load_fixture("rnnl_polar_32_16")
    N, K, L = int(d["N"]), int(d["K"]), int(d["curve_L"])
    code, info = code_of(N, K)
    net = net_of(sd, N, int(d["F"]), int(d["layers"]), 1)
    dec = RNN_decoder("y_input", N, info, onehot=True)
    snrs = [float(s) for s in d["curve_snr"]]
    n, nr = 1 << 14, int(d["curve_n"])
    mc = GRUListMonteCarlo(code, net, dec, L, snrs, n, n, seed=2031)
    res = mc.run()
    greedy = GRUMonteCarlo(code, net, dec, snrs, n, n, seed=2031).run()
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
        print(f"{s} dB L = {L}: BLER {p:.4f} (reference {pr:.4f}, z {z_bler:.2f}), BER z {z_ber:.2f}, "
              f"greedy BLER {float(greedy.bler[si]):.4f}")
        assert abs(z_bler) < 4 and abs(z_ber) < 4, (s, p, pr, z_bler, z_ber)
        assert p < float(greedy.bler[si]), (s, p, float(greedy.bler[si]))


# ------------------------------------------------------------------------------------------------ the rest
def test_graph_capture_and_replay_equal_eager():
    code, info, net, dec, y_all = shape_setup("polar_64_32_f64_l2")
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
    code, info, net, dec, y_all = shape_setup("polar_32_16_f64_l1")
    N, K, Ls = 32, 16, 4
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
    other = code_of(16, 8)[0].code
    assert lib.npd_gru_list_decode(h.h, other.h, p(y), None, Ls, p(hat2), None, None, None, B, s) == -1
    assert lib.npd_gru_list_supported(h.h, ch.h, Ls) == 1 and lib.npd_gru_list_supported(h.h, other.h, Ls) == 0
    assert lib.npd_gru_list_supported(h.h, ch.h, 9) == 0
    torch.cuda.synchronize()


def test_use_ynn_feeds_fy_and_selects_on_y():
    """--use_ynn: the GRU sees Fy = get_Fy(y), the selection the raw y.  Invariants 3 and 4."""
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
    assert np.array_equal(info, np.sort(d["info"]))
    dec = RNN_decoder("y_input", N, info, onehot=bool(d["onehot"]))
    y = torch.from_numpy(d["y"]).to(DEV)
    B, L = y.shape[0], 4
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
    clear = ds[:, 1] - ds[:, 0] >= H.DIST_MARGIN
    assert clear.mean() > 0.9
    assert np.array_equal(sel.cpu().numpy()[clear], dist.argmin(1)[clear])


def test_unsupported_handles_return_enotsup():
    from neural_polar_decoder_amd import _lib
    from neural_polar_decoder_amd.rnn import RNN_decoder, RNN_Model
    code, info = code_of(16, 8)
    N, K = 16, 8
    y = torch.zeros(4, N, device=DEV)
    hat = torch.zeros(4, K, device=DEV)
    lib = _lib.load()
    nets = [
        (RNN_Model("LSTM", N + 2, 32, 1, 1, N, 0, 0), "fp32"),
        (RNN_Model("GRU", N + 2, 128, 1, 1, N, 0, 0), "fp32"),
        (RNN_Model("GRU", N + 2, 32, 1, 2, N, 0, 0), "fp16x3"),
        (RNN_Model("GRU", N + 2, 32, 1, 2, N, 0, 0, use_layernorm=True), "fp32"),
        (RNN_Model("GRU", N + 2, 32, 1, 2, N, 32, 0, out_linear_depth=2), "fp32"),
    ]
    for net, precision in nets:
        net = net.to(DEV).eval()
        dec = RNN_decoder("y_input", N, info, onehot=True, precision=precision)
        assert not dec.list_supported(net, 4)
        with pytest.raises(_lib.NpdError):
            dec.list_decode(net, y, code, 4)
        h = dec._handle(net, y.device)  # the handle itself exists (the greedy decoder runs it); the list kernel refuses it
        assert lib.npd_gru_list_supported(h.h, code.code.h, 4) == 0
        rc = lib.npd_gru_list_decode(h.h, code.code.h, _lib.ptr(y), None, 4, _lib.ptr(hat), None, None, None, 4,
                                     _lib.stream_of(y.device))
        assert rc == -2, (type(net.rnn).__name__, precision, rc)
    torch.cuda.synchronize()
