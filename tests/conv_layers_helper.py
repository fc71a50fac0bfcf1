"""Shared by tests/test_conv_layers.py (CPU) and tests/test_conv_layers_gpu.py: the per-layer check of the convNet
kernels (npd_conv*.hip) against float64.

The logits sit behind three Linear layers and a LayerNorm, so a defect in one conv layer that is hundreds of times that
layer's own fp32 rounding still moves them by less than the 1e-5 logit bar (tests/test_conv_layers.py keeps that on
record).  Here every one of the 13 activations npd_conv_forward_tap can write (conv layers 0 .. 9, then the three Linear
outputs) is held to a bar anchored to the error of a plain fp32 evaluation of the same net:

    e_kernel = |kernel - float64|,  e_ref = |torch CPU fp32 - float64|   (same words, same weights)
    max(e_kernel) <= M max(e_ref)   and   p99(e_kernel) <= M p99(e_ref)   for every tap and for the logits.

M = 8, the cap: the smallest emulated defect (torch_forward) is 27 x e_ref at the maximum and 60 x at p99 (a residual
layer, where the residual's own rounding dominates e_ref), everything else 400 - 900 x.

Measured on an MI355X (256 CUs), largest e_kernel / e_ref over maximum and p99, per row and precision: the worst tap
besides the FC0 output, then the FC0 output (tap 10) as maximum / p99:

    row         fp32: worst other tap    FC0 output    fp16x3: worst other tap    FC0 output
    (32,64)     1.5 (tap 11)             2.1 / 2.1     1.4 (tap 11)               2.0 / 2.0
    (48,64)     1.7 (tap 7)              2.3 / 1.9     1.9 (tap 4)                3.0 / 2.1
    (112,64)    3.8 (tap 5)              1.7 / 2.0     1.7 (tap 9)                4.0 / 3.2
    (256,64)    5.6 (tap 1)              2.5 / 2.5     2.4 (tap 9)                4.0 / 3.1
    (32,128)    1.5 (tap 11)             1.7 / 1.8     1.5 (tap 11)               2.7 / 2.7
    (48,128)    1.9 (tap 9)              1.8 / 1.9     1.5 (tap 11)               3.6 / 3.1
    (112,128)   3.4 (tap 2)              2.1 / 1.8     1.5 (tap 9)                3.3 / 2.8
    (160,128)   3.4 (tap 9)              2.0 / 2.1     2.8 (tap 2)                2.9 / 2.7
    (160,192)   4.1 (tap 8)              1.6 / 1.9     2.3 (tap 4)                2.5 / 2.5
    (32,192)    1.6 (tap 11)             2.6 / 1.9     1.9 (tap 11)               5.5 / 3.2
    (48,192)    2.3 (tap 9)              2.3 / 1.9     1.8 (tap 11)               5.8 / 3.4
    (64,320)    2.2 (tap 9)              1.6 / 1.6     1.8 (tap 11)               2.7 / 2.6
    (32,384)    1.7 (tap 11)             1.6 / 1.8     2.1 (tap 11)               3.9 / 3.1
    (512,128)   7.6 (tap 2)              2.7 / 2.6     5.4 (tap 3)                2.9 / 2.4

Twice the largest ratio would be 16, so M stays at its cap and the ratios above 4 are findings, all of one kind: the
length of one fp32 accumulation chain, whose rounding grows about as sqrt(K), against torch's blocked GEMM and
convolution, whose error stays near the rounding of the result itself.  Conv layers sum K = 7 cin terms in one
chain: 5.6 - 7.6 only at cin 128 - 256 (K 896 - 1792) on the fp32 path, 5.4 at cin 256 in fp16x3.  The FC0 output (K = embed N) was the first
tap to leave the bar, with one chain over all of K: 8.7 - 14.5 x in fp32 from K = 12288 up, 11.3 x in fp16x3 at
K = 65536 (7.0 - 7.9 at K = 9216 - 30720); a sequential fp32 sum of its products on the CPU gave the same error
(1.0e-7 at K = 65536 against the fp32 kernel's 1.3e-7).  The FC kernels now end a chain every 1024 terms (fc_kernel)
or 8160 terms (fc_split_wsp_kernel) and add the chains' sums, which gives the figures above; the 5.5 - 5.8 left in
fp16x3 are K = 6144 and 9216, one chain of up to 8160 terms.
"""
import argparse
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conftest import conv_weights_from_seed

M = 8
ATOL = 1e-5          # the logit bar of tests/test_conv_gpu.py, kept beside the per-layer one
N_TAPS = 13
DILS = (1, 2, 4, 1, 2, 4, 1, 2, 4, 1)
CONV_NAMES = ("layers1.0", "layers1.2", "layers2.0", "layers2.2", "layers3.0", "layers3.2", "layers4.0", "layers4.2",
              "layers5.0", "layers5.2")
RES_FROM = {3: 1, 5: 3, 7: 5}  # layer -> the layer whose output is added after its GELU

# (embed, N): the kernel variants of npd_conv_forward_tap's dispatch the row reaches (fp16x3 unless said otherwise;
# ws = conv_split_ws_kernel<NG, Q, KS, NW>, ws16 = conv_ws16_kernel<KB, Q, NW, KP>, slab = conv_layer_split_kernel<P>)
ROWS = [
    (32, 64),    # ws<1,1> at cin exactly 16; ws16<1,1> with a half-filled 64-channel slice (layer 9, 32 outputs)
    (48, 64),    # ws<2,1> (cin 24), ws<3,1> (cin 48)
    (112, 64),   # ws<4,1,2,4> (cin 56, pad channels 56 -> 64); 112 outputs = 2 slices, the second ragged; slab P = 1, cin 112
    (256, 64),   # ws16<4,1,8,2> at dilations 1, 2, 4 with residual, 2 and 4 slices; slab at cin 256
    (32, 128),   # ws<1,2>, ws16<1,2>: 128-position items
    (48, 128),   # ws<2,2>, ws<3,2>
    (112, 128),  # ws<4,1,2,4> with 2 items per word
    (160, 128),  # slab P = 2 at cin 80 and 160, all dilations, residual
    (160, 192),  # slab P = 2 with a ragged last tile; 64 x 64 FC kernel with 3 column tiles
    (32, 192),   # Q = 1 with 3 items per word: ws<1,1>, ws16<1,1>
    (48, 192),   # Q = 1 with 3 items per word: ws<2,1>, ws<3,1>
    (64, 320),   # ws16<1,1>, ws16<2,1> with 5 items per word; 64 x 64 FC kernel with 5 column tiles
    (32, 384),   # all three Linear layers on the ring kernel with K blocks = 0 mod 3
    (512, 128),  # slab at cin 256, dilation 4 (160,512 of 163,840 LDS bytes at P = 2); layer 9 at cin 512 falls to
                 # P = 1 by the LDS test; the fp32 conv kernel at 144,480 B
]
SMALL_ROWS = [(48, 64), (256, 64), (160, 128)]  # the CPU clean run and the negative controls


def batch_of(E, N):
    """Words per row: every persistent layer gets >= 3 items per block and a ragged last round on a 256-CU device
    (asserted from the device's CU count by the GPU test, persistent_layers); (512, 128) has no persistent layer."""
    if E == 512:
        return 67
    return 1700 if N == 64 else 850


def compare_words(E, N):
    """The words compared against float64: word 0, the last word and words spread over every round in between."""
    B = batch_of(E, N)
    n = 4 if E == 512 else 12
    return np.unique(np.round(np.linspace(0, B - 1, n)).astype(np.int64))


def row_weights(E, N):
    return conv_weights_from_seed(E, N, 100 + E)


def row_words(E, N, B=None):
    rng = np.random.default_rng(E + N)
    B = batch_of(E, N) if B is None else B
    return (np.where(rng.random((B, N)) < 0.5, -1.0, 1.0) + 0.8 * rng.standard_normal((B, N))).astype(np.float32)


def persistent_layers(E, N, B, cu):
    """The fp16x3 dispatch's weight-stationary layers of one chunk of B words: (layer, kernel, items per block column,
    block columns) -- a block column walks items j, j + columns, ...; an item is 64 Q positions of one word."""
    out = []
    for i in range(1, 10):
        cin = E if i == 9 else E // 2
        cout = E if i >= 8 else E // 2
        nsl = (cout + 63) // 64
        if cin in (32, 64, 128):
            kb = cin // 32
            Q = 2 if kb < 4 and N % 128 == 0 else 1
            name, nblk = f"ws16<{kb},{Q}>", cu
        elif cin <= 64:
            ng = (cin + 15) // 16
            Q = 2 if ng <= 3 and N % 128 == 0 else 1
            name, nblk = f"ws<{ng},{Q}>", cu * (2 if ng == 4 else 1)
        else:
            continue
        items = B * (N // (64 * Q))
        nblk -= nblk % nsl
        nblk = max(min(nblk, items * nsl), nsl)
        out.append((i, name, items, nblk // nsl))
    return out


def net_from(sd, embed, N, precision="fp32", bias=True):
    from neural_polar_decoder_amd.models import convNet
    cfg = argparse.Namespace(embed_dim=embed, max_len=N, N=N, dont_use_bias=not bias, dropout=0.0)
    net = convNet(cfg, precision=precision)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.eval()


def kernel_taps(net, y, sel):
    """All 13 taps, the logits and the decisions of the product kernels for the words y (device tensor), at rows sel;
    one forward per tap, each of which must give the same logits and decisions."""
    taps, lg0, dec0 = [], None, None
    for t in range(N_TAPS):
        lg, dec, a = net.logits(y, tap=t)
        assert a.shape == net.tap_shape(t, y.shape[0])
        if lg0 is None:
            lg0, dec0 = lg, dec
        else:
            assert torch.equal(lg, lg0) and torch.equal(dec, dec0), ("logits differ between tap calls", t)
        taps.append(a[torch.as_tensor(sel, device=a.device)].cpu().numpy())
    return taps, lg0.cpu().numpy()[sel], dec0.cpu().numpy()[sel]


# ------------------------------------------------------------------------------ torch CPU fp32 restatement
def torch_forward(y, sd, defect=None):
    """convNet.forward (models.py:742-767) in torch CPU fp32: (logits, the 13 activations) as numpy float32.

    defect = (kind, layer) emulates a kernel defect in conv layer `layer`:
      "act16"  its input activations rounded to fp16 (a dropped lo product of the activation split),
      "w16"    its weights rounded to fp16 (a dropped lo product of the weight split),
      "drop"   output channel 1 at position N / 2 + 1 reads input channel 0 at that position (its centre tap) as zero:
               one output element per word misses one of its 7 cin products, the smallest index slip there is."""
    kind, at = defect if defect is not None else (None, -1)
    taps = []
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(y, np.float32))[:, None, :]
        for i, name in enumerate(CONV_NAMES):
            w = torch.from_numpy(np.asarray(sd[name + ".weight"], np.float32))
            b = sd.get(name + ".bias")
            b = None if b is None else torch.from_numpy(np.asarray(b, np.float32))
            xin = x
            if i == at and kind == "act16":
                xin = x.half().float()
            if i == at and kind == "w16":
                w = w.half().float()
            o = F.conv1d(xin, w, b, padding=3 * DILS[i], dilation=DILS[i])
            if i == at and kind == "drop":
                l0 = x.shape[2] // 2 + 1
                xz = x.clone()
                xz[:, 0, l0] = 0.0
                o[:, 1, l0] = F.conv1d(xz, w, b, padding=3 * DILS[i], dilation=DILS[i])[:, 1, l0]
            o = F.gelu(o)
            if i in RES_FROM:
                o = o + torch.from_numpy(taps[RES_FROM[i]])
            taps.append(o.numpy())
            x = o
        h = x.reshape(x.shape[0], -1)
        for j, li in enumerate((0, 2, 4)):
            h = F.linear(h, torch.from_numpy(np.asarray(sd[f"layersFin.{li}.weight"], np.float32)),
                         torch.from_numpy(np.asarray(sd[f"layersFin.{li}.bias"], np.float32)))
            if j < 2:
                h = F.gelu(h)
            taps.append(h.numpy())
        n = h.shape[1]
        lg = F.layer_norm(h, (n,), torch.from_numpy(np.asarray(sd["layer_norm.weight"], np.float32)),
                          torch.from_numpy(np.asarray(sd["layer_norm.bias"], np.float32)), eps=1e-6)
    return lg.numpy(), taps


class Reference:
    """float64 (oracle.conv_forward) and torch fp32 activations and logits of the same words."""

    def __init__(self, oracle, y, sd):
        self.lg64, self.taps64 = oracle.conv_forward(y, sd, out_dtype=np.float64, want_taps=True)
        self.lg32, self.taps32 = torch_forward(y, sd)

    def skip_share(self):
        """Share of the logits the sign check leaves out as within ATOL of zero."""
        return float((np.abs(self.lg64) <= ATOL).mean())


@functools.lru_cache(maxsize=None)
def _row_reference(E, N):
    from oracle import oracle as O
    O.lib()
    return Reference(O, row_words(E, N)[compare_words(E, N)], row_weights(E, N))


def row_reference(E, N):
    """The row's Reference on its compare words: computed once, shared by every test of the row, never written to."""
    return _row_reference(E, N)


# ------------------------------------------------------------------------------------------------ the checks
def tap_ratios(taps, lg, ref):
    """[(name, max e_kernel, max e_ref, p99 e_kernel, p99 e_ref)] for the 13 taps and the logits."""
    rows = []
    for name, k, r32, r64 in [(f"tap{t}", taps[t], ref.taps32[t], ref.taps64[t]) for t in range(N_TAPS)] + \
                             [("logits", lg, ref.lg32, ref.lg64)]:
        assert k.shape == r64.shape, (name, k.shape, r64.shape)
        assert np.isfinite(k).all(), name
        ek = np.abs(k.astype(np.float64) - r64).ravel()
        er = np.abs(r32.astype(np.float64) - r64).ravel()
        rows.append((name, ek.max(), er.max(), np.percentile(ek, 99), np.percentile(er, 99)))
    return rows


def worst_ratio(rows):
    """(ratio, name) of the largest e_kernel / e_ref over max and p99 (0 / 0 counts as 0)."""
    best = (0.0, "")
    for name, km, rm, kp, rp in rows:
        for a, b in ((km, rm), (kp, rp)):
            r = 0.0 if a == 0 else (np.inf if b == 0 else a / b)
            if r > best[0]:
                best = (float(r), name)
    return best


def check_logits_only(lg, dec, ref_lg):
    """The bar of tests/test_conv_gpu.py: logits within 1e-5, decisions identical away from zero."""
    err = np.abs(lg - ref_lg).max()
    assert err < ATOL, ("max |logit diff|", float(err))
    sure = np.abs(ref_lg) > ATOL
    assert np.array_equal(dec[sure], np.sign(ref_lg)[sure])


FC0 = "tap10"
BESIDES_FC0 = tuple(f"tap{t}" for t in range(N_TAPS) if t != 10) + ("logits",)


def check_taps(taps, lg, dec, ref, m=M, label="", names=None):
    """Every tap and the logits (or those in `names`) within m x the fp32 restatement's own error against float64, at
    the maximum and at p99; and the logit bar and sign check of tests/test_conv_gpu.py.  Prints every figure first and
    reports every miss in one assertion.  Returns tap_ratios."""
    rows = tap_ratios(taps, lg, ref)
    for name, km, rm, kp, rp in rows:
        print(f"{label} {name}: max {km:.3e} / {rm:.3e}  p99 {kp:.3e} / {rp:.3e}")
    print(f"{label} worst ratio {worst_ratio(rows)}")
    missed = []
    for name, km, rm, kp, rp in rows:
        if names is not None and name not in names:
            continue
        if km > m * rm:
            missed.append((name, "max", float(km), float(rm)))
        if kp > m * rp:
            missed.append((name, "p99", float(kp), float(rp)))
    assert not missed, (label, "e_kernel > m e_ref", m, missed)
    if names is None or "logits" in names:
        check_logits_only(lg, dec, ref.lg64)
    return rows
