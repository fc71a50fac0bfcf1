"""Helpers of the GRU list-decoding tests (tests/test_rnnl.py, tests/test_rnnl_gpu.py).

``list_decode_np`` restates RNN_decoder.list_decode (rnn_all.py:563-664, decoding_type y_input) in numpy, in float64 by
default: one GRU step per live path and position (PyTorch GRUCell: gates r, z, n; h' = (1 - z) n + z h), a fork at every
information position (child l keeps sign(out_l) and its metric, child ls + l takes -sign(out_l) and metric + |out_l|),
pruneLists = the L smallest metrics in ascending child index, and the first minimum of ||encode(msg) - y||^2 over the
survivors.  ``encode_np`` is the code's encoder over GF(2) (Polar: Plotkin butterfly; PAC: rate-1 convolution first).
The fixtures (tests/golden/gen_rnnl.py) record the reference's own results; this restatement pins what they mean.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

LOGIT_ATOL = 2e-5   # the project's fp32 logit tolerance (tests/test_gru_gpu.py)
DIST_MARGIN = 1e-3  # above N 2^-24 distance (~4e-4 at N = 64, distance 100)

# fixture -> (source of the weights: a trained fixture's name, or None when the fixture stores them; list sizes)
# trained_crisp_64_32 (the hidden-64 Polar(64,32) net that never learned to decode, BLER ~ 1) gives no fixture: its
# paths' metrics sit too close for the robust-share condition at every SNR tried (gen_rnnl.py).  K = 32 with two bit
# words is covered by a seeded, scaled Polar(64,32) net instead, regenerated from its torch seed.
FIXTURES = {
    "rnnl_polar_32_16": ("trained_crisp_32_16", (2, 3, 4, 8)),
    "rnnl_polar_64_32_seeded": (None, (4, 8)),
    "rnnl_pac_32_10": ("trained_pac_32_10", (4,)),
    "rnnl_polar_16_8_f32_l1": (None, (2, 5)),
}


def seeded_state_dict(N, F, layers, onehot, w_seed, gru_scale, lin_scale):
    """A seeded net's weights: RNN_Model's PyTorch-default draws under torch.manual_seed(w_seed) (the same parameter
    draws as the reference's RNN_Model), GRU parameters times gru_scale and the output Linear's times lin_scale."""
    import torch
    from neural_polar_decoder_amd.rnn import RNN_Model
    torch.manual_seed(int(w_seed))
    net = RNN_Model("GRU", N + 1 + int(onehot), F, 1, layers, N, 0, 0, "selu", 0.0, False, out_linear_depth=1)
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.mul_(float(gru_scale) if k.startswith("rnn.") else float(lin_scale))
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


def weights_digest(sd):
    """sha256 over a state dict's arrays in sorted key order (as tests/conftest.py)."""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], np.float32).tobytes())
    return h.hexdigest()


def load_fixture(name):
    """(fixture, state dict of its net): weights stored in the fixture, or taken from the trained fixture it names and
    checked against the stored digest."""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    if "w_source" in d.files:
        src = np.load(os.path.join(GOLDEN, bytes(d["w_source"]).decode() + ".npz"))
        sd = {k[2:]: np.asarray(src[k]) for k in src.files if k.startswith("w.")}
    elif "w_seed" in d.files:
        sd = seeded_state_dict(int(d["N"]), int(d["F"]), int(d["layers"]), int(d["onehot"]), int(d["w_seed"]),
                               *d["w_scale"])
    else:
        sd = {k[2:]: np.asarray(d[k]) for k in d.files if k.startswith("w.")}
    assert weights_digest(sd) == bytes(d["w_digest"]).decode(), "the fixture's net is not the one it was generated with"
    return d, sd


def unpack_pm1(bits, K):
    """bit-packed (.., ceil(K / 8)) -> +-1 float32 (.., K); a set bit is -1."""
    b = np.unpackbits(bits, axis=-1)[..., :K]
    return np.where(b == 1, -1.0, 1.0).astype(np.float32)


def pac_taps(g):
    """(tap mask, state mask) of the PAC convolution polynomial g: g_array[j] (MSB first) taps state[j - 1]."""
    M = int(g).bit_length()
    tap = 0
    for j in range(1, M):
        if (int(g) >> (M - 1 - j)) & 1:
            tap |= 1 << (j - 1)
    return tap, (1 << (M - 1)) - 1


def encode_np(msg, N, info, pac_g=0):
    """+-1 messages (M, K) -> +-1 codewords (M, N), float64: u[info] = msg, PAC convolution u_i = v_i ^ parity(state &
    taps), state <- v (pac_code.py:181-208), Plotkin butterfly (polar.py:128-148)."""
    msg = np.asarray(msg)
    M = msg.shape[0]
    v = np.zeros((M, N), np.int64)
    v[:, np.sort(np.asarray(info, np.int64))] = (msg < 0).astype(np.int64)
    u = v.copy()
    if pac_g:
        tap, smask = pac_taps(pac_g)
        st = np.zeros(M, np.int64)
        for i in range(N):
            par = np.zeros(M, np.int64)
            x = st & tap
            while np.any(x):
                par ^= x & 1
                x = x >> 1
            u[:, i] = v[:, i] ^ par
            st = ((st << 1) | v[:, i]) & smask
    h = 1
    while h < N:
        u = u.reshape(M, N // (2 * h), 2, h)
        u[:, :, 0, :] ^= u[:, :, 1, :]
        u = u.reshape(M, N)
        h *= 2
    return 1.0 - 2.0 * u.astype(np.float64)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gru_step_np(sd, layers, x, h):
    """One step of nn.GRU(batch_first) + Linear(F, 1): x (M, Din), h (layers, M, F) -> out (M), new h."""
    hn = []
    inp = x
    for l in range(layers):
        wih, whh = sd[f"rnn.weight_ih_l{l}"], sd[f"rnn.weight_hh_l{l}"]
        bih, bhh = sd[f"rnn.bias_ih_l{l}"], sd[f"rnn.bias_hh_l{l}"]
        F = whh.shape[1]
        gi = inp @ wih.T + bih
        gh = h[l] @ whh.T + bhh
        r = _sigmoid(gi[:, :F] + gh[:, :F])
        z = _sigmoid(gi[:, F:2 * F] + gh[:, F:2 * F])
        n = np.tanh(gi[:, 2 * F:] + r * gh[:, 2 * F:])
        inp = (1.0 - z) * n + z * h[l]
        hn.append(inp)
    out = inp @ sd["linear.weight"].reshape(-1) + sd["linear.bias"].reshape(-1)[0]
    return out, np.stack(hn)


def list_decode_np(sd, N, info, onehot, layers, y, L, pac_g=0, fy=None, dtype=np.float64):
    """list_decode in numpy.  Returns a dict: msg (B, K) +-1, sel (B), cand_msg (B, ls, K), cand_metric (B, ls), dist
    (B, ls), prune_margin (B) = min over prune events of the (L+1)-th smallest metric minus the L-th (inf if none),
    dist_margin (B) = second smallest final distance minus the smallest (inf for a single survivor)."""
    sd = {k: np.asarray(v, dtype) for k, v in sd.items()}
    y = np.asarray(y, dtype)
    fy = y if fy is None else np.asarray(fy, dtype)
    info = np.sort(np.asarray(info, np.int64))
    isinfo = np.zeros(N, bool)
    isinfo[info] = True
    B = y.shape[0]
    F = sd["rnn.weight_hh_l0"].shape[1]
    hid = np.zeros((1, layers, B, F), dtype)      # (list, layers, B, F)
    dec = np.ones((1, B, N), dtype)
    met = np.zeros((1, B), dtype)
    rows = np.arange(B)
    margin = np.full(B, np.inf)
    for ii in range(N):
        ls = hid.shape[0]
        outs = np.zeros((ls, B), dtype)
        newh = np.zeros_like(hid)
        for l in range(ls):
            prev = np.ones(B, dtype) if ii == 0 else np.sign(dec[l, :, ii - 1])
            if onehot:  # get_onehot (rnn_all.py:258-260): column index (0.5 + 0.5 s)
                idx = (0.5 + 0.5 * prev).astype(np.int64)
                xin = np.concatenate([fy, np.eye(2, dtype=dtype)[idx]], 1)
            else:
                xin = np.concatenate([fy, prev[:, None]], 1)
            outs[l], newh[l] = gru_step_np(sd, layers, xin, hid[l])
        if not isinfo[ii]:
            hid = newh
            continue
        hid = np.concatenate([newh, newh], 0)
        dec = np.concatenate([dec, dec], 0)
        dec[:ls, :, ii] = np.sign(outs)
        dec[ls:, :, ii] = -np.sign(outs)
        met = np.concatenate([met, met + np.abs(outs)], 0)
        if 2 * ls > L:
            order = np.argsort(met, axis=0, kind="stable")
            srt = np.take_along_axis(met, order, 0)
            margin = np.minimum(margin, srt[L] - srt[L - 1])
            keep = np.sort(order[:L], axis=0)
            hid = hid[keep, :, rows].transpose(0, 2, 1, 3)  # (L, B, layers, F) -> (L, layers, B, F)
            met = met[keep, rows]
            dec = dec[keep, rows]
    ls = dec.shape[0]
    cand = dec[:, :, info]
    cwd = encode_np(cand.reshape(ls * B, -1), N, info, pac_g).reshape(ls, B, N)
    dist = ((cwd - y[None]) ** 2).sum(2)
    sel = dist.argmin(0)
    ds = np.sort(dist, 0)
    return {"msg": cand[sel, rows], "sel": sel, "cand_msg": cand.transpose(1, 0, 2), "cand_metric": met.T,
            "dist": dist.T, "prune_margin": margin,
            "dist_margin": ds[1] - ds[0] if ls > 1 else np.full(B, np.inf)}


def robust_mask(d, L):
    """Words of a fixture whose list decoding cannot turn on fp32 rounding: every prune boundary wider than two metrics'
    tolerance (each a sum of at most K logits held to LOGIT_ATOL) and the final selection wider than DIST_MARGIN."""
    K = int(d["K"])
    return (d[f"prune_margin_L{L}"] >= 2 * K * LOGIT_ATOL) & (d[f"dist_margin_L{L}"] >= DIST_MARGIN)


def sorted_candidates(cand_msg, cand_metric):
    """Per word, the candidates in a canonical order, for comparing survivor SETS: by message (messages of a list are
    distinct, so this orders them fully), the metric only as a last key.  Ordering by metric first would let two
    metrics inside the tolerance of each other swap places between two fp32 implementations of the same set."""
    B, L, K = cand_msg.shape
    out_m = np.empty_like(cand_msg)
    out_t = np.empty_like(cand_metric)
    for b in range(B):
        keys = [cand_metric[b]] + [cand_msg[b, :, k] for k in range(K - 1, -1, -1)]
        o = np.lexsort(keys)
        out_m[b], out_t[b] = cand_msg[b, o], cand_metric[b, o]
    return out_m, out_t
