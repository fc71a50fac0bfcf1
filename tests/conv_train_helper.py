"""float64 restatement of convNet training -- models.convNet.forward in training mode (models.py:742-767) and the
gradient of sum(grad_logits * logits) -- written out layer by layer (no autograd), for tests/test_conv_train.py (CPU:
against fixtures recorded from the reference, tests/golden/gen_conv_train.py) and tests/test_conv_train_gpu.py (the
fused kernels, npd_conv_train_forward / _backward).

Activations are channels-first (B, C, N) as in the reference; the dropout layer is a given multiplier `drop` (B, N) of 0
or 1 / (1 - p), or None.  Gradients come back by state-dict name in the reference's shapes.

The gradient bar (tests/train_helper.py's): every tensor, and every block of blocks(), within GRAD_FACTOR * E_ref of the
float64 gradient relative to that gradient's norm, E_ref being torch's fp32 CPU autograd (torch_train) on the same
inputs measured the same way.

MUTATIONS are wrong variants of the restatement, each a plausible kernel defect; each must miss a case's bar by a wide
margin, so the bar tells a defect from rounding.
"""
import collections
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = "conv_train_64_e16"
GRAD_FACTOR = 16.0
DILS = (1, 2, 4, 1, 2, 4, 1, 2, 4, 1)
CONV_NAMES = ("layers1.0", "layers1.2", "layers2.0", "layers2.2", "layers3.0", "layers3.2", "layers4.0", "layers4.2",
              "layers5.0", "layers5.2")
FC_NAMES = ("layersFin.0", "layersFin.2", "layersFin.4")
RES_FROM = {3: 1, 5: 3, 7: 5}  # layer -> the layer whose output is added after its GELU

# (name, applies(case)): where a mutation changes nothing by construction it is not asked to miss
MUTATIONS = (
    ("dx_no_flip", lambda c: True),            # dX with tap t's weights where tap 6 - t's belong
    ("dx_no_dilation", lambda c: True),        # dX with dilation 1 in every layer
    ("dw_halo_wrap", lambda c: True),          # dW reads positions past the ends modulo N instead of zeros
    ("skip_grad_dropped", lambda c: True),     # the gradient along layer 3's skip never reaches layer 1's output
    ("gelu_tanh", lambda c: True),             # GELU' of the tanh approximation
    ("ln_no_mean", lambda c: True),            # LayerNorm backward without its two mean terms
    ("drop_missing_bwd", lambda c: c.drop),    # the dropout multiplier left out of the backward
    ("fc0_dw_order", lambda c: True),          # FC0's dW left in the kernels' l E + c column order
    ("last_word_twice", lambda c: True),       # the last word counted twice in every weight and bias gradient
    ("tail_dropped", lambda c: True),          # the last two words missing from conv layer 4's dW
)

# (embed, N, B, use_bias, drop, info): tests/test_conv_train_gpu.py's cases, the smallest shapes at which each mechanism
# of the kernels can fail.  drop: a dropout multiplier (p = 0.25); info: grad_out zero outside a 22-position set.
Case = collections.namedtuple("Case", "embed N B bias drop info seed why")
CASES = (
    Case(16, 64, 1, True, False, False, 8101, "cin = 8, a single word"),
    Case(16, 64, 3, False, False, False, 8102, "absent biases"),
    Case(32, 64, 65, True, True, False, 8103, "one word past a 64-row FC tile; dropout"),
    Case(48, 64, 200, True, False, False, 8104, "cout = 24 padded into a 32-row tile, cin = 24"),
    Case(128, 64, 70, True, False, True, 8105, "run_alt.sh's width, cin 128 in layer 9; information-set grad_out"),
    Case(16, 128, 33, True, False, False, 8106, "two position tiles, the dilation-4 halo crossing their boundary"),
    Case(32, 256, 5, True, False, False, 8107, "four position tiles"),
)


def case_id(c):
    return f"e{c.embed}-n{c.N}-b{c.B}" + ("" if c.bias else "-nobias") + ("-drop" if c.drop else "") + \
        ("-info" if c.info else "")


def param_names(use_bias=True):
    names = []
    for n in CONV_NAMES:
        names += [n + ".weight"] + ([n + ".bias"] if use_bias else [])
    for n in FC_NAMES:
        names += [n + ".weight", n + ".bias"]
    return names + ["layer_norm.weight", "layer_norm.bias"]


def case_weights(c):
    """PyTorch-default-like draws (U(+-1/sqrt(fan_in)); LayerNorm 1 + 0.1 U, 0.1 U) under the case's seed, as
    conftest.conv_weights_from_seed; without the conv biases for a bias-free case."""
    from conftest import conv_weights_from_seed
    sd = conv_weights_from_seed(c.embed, c.N, c.seed)
    if not c.bias:
        sd = {k: v for k, v in sd.items() if not (k.startswith("layers") and k.endswith(".bias")
                                                   and not k.startswith("layersFin"))}
    return sd


def case_inputs(c):
    """y = +-1 + 0.8 N(0, 1), the dropout multiplier or None, and grad_out (B, N)."""
    rng = np.random.default_rng(c.seed + 1)
    y = (np.where(rng.random((c.B, c.N)) < 0.5, -1.0, 1.0) + 0.8 * rng.standard_normal((c.B, c.N))).astype(np.float32)
    drop = ((rng.random((c.B, c.N)) >= 0.25) / 0.75).astype(np.float32) if c.drop else None
    gout = rng.standard_normal((c.B, c.N)).astype(np.float32)
    if c.info:
        keep = np.zeros(c.N, np.float32)
        keep[np.sort(rng.permutation(c.N)[:22])] = 1.0
        gout = gout * keep
    return y, drop, gout


# ---------------------------------------------------------------------------------- the restatement
def _erf(x):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def gelu(z):
    return 0.5 * z * (1.0 + _erf(z / np.sqrt(2.0)))


def gelu_grad(z, mutation=None):
    if mutation == "gelu_tanh":
        k = np.sqrt(2.0 / np.pi)
        u = k * (z + 0.044715 * z ** 3)
        t = np.tanh(u)
        return 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * k * (1.0 + 3 * 0.044715 * z * z)
    return 0.5 * (1.0 + _erf(z / np.sqrt(2.0))) + z * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


def _pad(x, p, wrap=False):
    return np.pad(x, ((0, 0), (0, 0), (p, p)), mode="wrap" if wrap else "constant")


def forward64(sd, y, drop=None):
    """logits (B, N) and the cache for backward64."""
    W = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    y = np.asarray(y, np.float64)
    B, N = y.shape
    x = y[:, None, :]
    xs, zs, outs = [], [], []
    for i, name in enumerate(CONV_NAMES):
        w, d = W[name + ".weight"], DILS[i]
        xp = _pad(x, 3 * d)
        z = np.zeros((B, w.shape[0], N))
        for t in range(7):
            z += w[:, :, t] @ xp[:, :, d * t:d * t + N]
        if name + ".bias" in W:
            z += W[name + ".bias"][None, :, None]
        a = gelu(z)
        if i in RES_FROM:
            a = a + outs[RES_FROM[i]]
        xs.append(x), zs.append(z), outs.append(a)
        x = a
    h = x.reshape(B, -1)  # c N + l
    fx, fz = [], []
    for f, name in enumerate(FC_NAMES):
        z = h @ W[name + ".weight"].T + W[name + ".bias"]
        fx.append(h), fz.append(z)
        h = gelu(z) if f < 2 else z
    dd = h if drop is None else h * np.asarray(drop, np.float64)
    mean = dd.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(dd.var(1, keepdims=True) + 1e-6)
    xh = (dd - mean) * rstd
    logits = xh * W["layer_norm.weight"] + W["layer_norm.bias"]
    return logits, dict(W=W, xs=xs, zs=zs, fx=fx, fz=fz, xh=xh, rstd=rstd, drop=drop, B=B, N=N)


def backward64(cx, gout, mutation=None):
    """Gradients (float64, by state-dict name) of sum(gout * logits)."""
    W, B, N = cx["W"], cx["B"], cx["N"]
    gout = np.asarray(gout, np.float64)
    g = {}
    wrow = np.ones(B)
    if mutation == "last_word_twice":
        wrow[-1] = 2.0
    wr = wrow[:, None]
    xh, rstd = cx["xh"], cx["rstd"]
    g["layer_norm.weight"] = (gout * xh * wr).sum(0)
    g["layer_norm.bias"] = (gout * wr).sum(0)
    a = gout * W["layer_norm.weight"]
    if mutation == "ln_no_mean":
        dz = rstd * a
    else:
        dz = rstd * (a - a.mean(1, keepdims=True) - xh * (a * xh).mean(1, keepdims=True))
    if cx["drop"] is not None and mutation != "drop_missing_bwd":
        dz = dz * np.asarray(cx["drop"], np.float64)
    for f in (2, 1, 0):
        name = FC_NAMES[f]
        dw = (dz * wr).T @ cx["fx"][f]
        if f == 0 and mutation == "fc0_dw_order":
            C = cx["zs"][9].shape[1]
            dw = dw.reshape(-1, C, N).transpose(0, 2, 1).reshape(dw.shape)
        g[name + ".weight"] = dw
        g[name + ".bias"] = (dz * wr).sum(0)
        dx = dz @ W[name + ".weight"]
        dz = dx * gelu_grad(cx["fz"][f - 1], mutation) if f > 0 else dx
    G = {9: dz.reshape(B, -1, N)}  # the whole gradient at each conv layer's output
    for i in range(9, -1, -1):
        name, d = CONV_NAMES[i], DILS[i]
        w = W[name + ".weight"]
        dZ = G[i] * gelu_grad(cx["zs"][i], mutation)
        xp = _pad(cx["xs"][i], 3 * d, wrap=mutation == "dw_halo_wrap")
        wc = wrow.copy()
        if mutation == "tail_dropped" and i == 4:
            wc[-2:] = 0.0
        dZw = dZ * wc[:, None, None]
        dw = np.zeros_like(w)
        for t in range(7):
            dw[:, :, t] = np.tensordot(dZw, xp[:, :, d * t:d * t + N], axes=([0, 2], [0, 2]))
        g[name + ".weight"] = dw
        if name + ".bias" in W:
            g[name + ".bias"] = (dZ * wr[:, :, None]).sum((0, 2))
        if i == 0:
            break
        dd = 1 if mutation == "dx_no_dilation" else d
        dxp = np.zeros((B, w.shape[1], N + 6 * dd))
        for t in range(7):
            wt = w[:, :, 6 - t] if mutation == "dx_no_flip" else w[:, :, t]
            dxp[:, :, dd * t:dd * t + N] += wt.T @ dZ
        G[i - 1] = G.get(i - 1, 0.0) + dxp[:, :, 3 * dd:3 * dd + N]
        if i in RES_FROM and not (mutation == "skip_grad_dropped" and i == 3):
            G[RES_FROM[i]] = G[i]  # out_i = gelu(z_i) + out_{i-2}: the whole gradient also arrives along the skip
    return g


def train64(sd, y, drop, gout, mutation=None):
    logits, cx = forward64(sd, y, drop)
    return logits, backward64(cx, gout, mutation)


# ---------------------------------------------------------------------------------- errors and blocks
def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def blocks(grads):
    """A gradient dict and, beside every whole tensor, the blocks different parts of the kernels fill: each of the 7
    taps of every conv weight (`name.tap3`) and FC0's weight by position l (`layersFin.0.weight.l17`)."""
    out = {}
    for k, v in grads.items():
        v = np.asarray(v)
        out[k] = v
        if k.endswith(".weight") and v.ndim == 3:
            for t in range(7):
                out[f"{k}.tap{t}"] = v[:, :, t]
        if k == "layersFin.0.weight":
            N = v.shape[0] // 4
            v3 = v.reshape(v.shape[0], -1, N)
            for l in range(N):
                out[f"{k}.l{l}"] = v3[:, :, l]
    return out


def block_errs(got, ref):
    gb, rb = blocks(got), blocks(ref)
    assert sorted(gb) == sorted(rb), sorted(set(gb) ^ set(rb))
    errs = {}
    for k, v in rb.items():
        assert np.linalg.norm(v.ravel()) > 0.0, f"gradient block {k} is zero"
        errs[k] = rel_err(gb[k], v)
    return errs


# ---------------------------------------------------------------------------------- torch autograd (E_ref, float64 check)
def torch_train(sd, y, drop, gout, dtype=torch.float32):
    """convNet's training forward in plain torch ops on the CPU and autograd's gradients of sum(gout * logits):
    (logits, grads by name) as float64 numpy."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    x = torch.as_tensor(np.asarray(y), dtype=dtype).unsqueeze(1)
    outs = []
    for i, name in enumerate(CONV_NAMES):
        a = F.gelu(F.conv1d(x, P[name + ".weight"], P.get(name + ".bias"), padding=3 * DILS[i], dilation=DILS[i]))
        if i in RES_FROM:
            a = a + outs[RES_FROM[i]]
        outs.append(a)
        x = a
    h = torch.flatten(x, start_dim=1)
    for f, name in enumerate(FC_NAMES):
        h = F.linear(h, P[name + ".weight"], P[name + ".bias"])
        if f < 2:
            h = F.gelu(h)
    if drop is not None:
        h = h * torch.as_tensor(np.asarray(drop), dtype=dtype)
    N = h.shape[1]
    logits = F.layer_norm(h, (N,), P["layer_norm.weight"], P["layer_norm.bias"], eps=1e-6)
    (logits * torch.as_tensor(np.asarray(gout), dtype=dtype)).sum().backward()
    return logits.detach().double().numpy(), {k: p.grad.detach().double().numpy().copy() for k, p in P.items()}


FIX_SEED = 8001                      # tests/golden/gen_conv_train.py's SEED, ROWS and proj
FIX_ROWS = np.arange(5, 256, 64)


def fix_view(grads):
    """A full gradient dict in the fixture's form: layersFin.0.weight as its recorded rows and its projection."""
    out = {k: np.asarray(v, np.float64) for k, v in grads.items() if k != "layersFin.0.weight"}
    g = np.asarray(grads["layersFin.0.weight"], np.float64)
    out["layersFin.0.weight.rows"] = g[FIX_ROWS]
    out["layersFin.0.weight.proj"] = np.random.default_rng(FIX_SEED + 2).standard_normal(g.shape[0]) @ g
    return out


def load_fixture():
    """tests/golden/conv_train_64_e16.npz: per mode ("plain", "drop") the weights (layersFin.0.weight from the seed,
    checked against the recorded sum), y, gout, [drop], logits32 / logits64 and the reference's gradients g32 / g64 in
    fix_view's form."""
    from conftest import conv_weights_from_seed
    d = np.load(os.path.join(GOLDEN, FIXTURE + ".npz"))
    w0 = conv_weights_from_seed(16, 64, FIX_SEED)["layersFin.0.weight"]
    assert float(w0.astype(np.float64).sum()) == float(d["w0sum"])
    sd = {k[2:]: d[k] for k in d.files if k.startswith("w.")}
    sd["layersFin.0.weight"] = w0
    fx = {}
    for mode in ("plain", "drop"):
        pre = mode + "."
        m = {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}
        fx[mode] = dict(sd=sd,
                        g32={k[4:]: v for k, v in m.items() if k.startswith("g32.")},
                        g64={k[4:]: v for k, v in m.items() if k.startswith("g64.")},
                        y=m["y"], gout=m["gout"], drop=m.get("drop"), logits32=m["logits32"], logits64=m["logits64"])
    return fx
