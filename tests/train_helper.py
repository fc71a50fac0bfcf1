"""float64 restatement of CRISP GRU training -- RNN_decoder.decode(net, True, y, gt, tfr) (rnn_all.py:422-512) and its
gradient -- written out explicitly (no autograd), for tests/test_gru_train.py (CPU, against fixtures recorded from the
reference), tests/test_gru_train_gpu.py (the fused kernels) and the SHAPE_CASES of tests/test_gru_train_shapes.py
(CPU) / tests/test_gru_train_shapes_gpu.py (long codes, large batches, saturated gates; the per-block metric).

Frames.  Everything here is in the step frame ii = 0 .. N-1; under reverse_order the caller flips gt on entry and the
result on return, as the reference does.  `bits` (B, N) is the fed path: bits[:, ii] is what step ii hands to step
ii + 1 (teacher forcing: gt[:, ii]; student forcing: sign(decoded[:, ii]), which is +1 wherever no logit was written);
step 0 is fed +1.  `writes` (N,) marks the steps whose logit goes into decoded (student forcing: ii in info_inds;
teacher forcing: every step); elsewhere decoded is the constant 1.0.

MUTATIONS are wrong variants of the restatement; each must miss a case's gradient bar by a wide margin, so the bar
tells a dropped term from rounding.
"""
import collections
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("train_gru_f32_l1_n16_rev", "train_gru_f64_l2_n16_onehot")
GRAD_FACTOR = 16.0   # gradient bar = GRAD_FACTOR * E_ref (E_ref: torch's fp32 autograd against this restatement)
LOGIT_BAR = 2e-5     # the project's fp32 GRU logit bar (forced_helper.bar_of)
# (name, applies(student, rev)): where a mutation changes nothing by construction it is not asked to miss
MUTATIONS = (
    ("bhn_outside", lambda student, rev: True),          # n = tanh(a_in + r (W_hn h) + b_hn)
    ("dahn_no_r", lambda student, rev: True),            # da_hn = da_n
    ("no_carry", lambda student, rev: True),             # dh_prev = W_hh^T Delta_hh, without dh z
    ("dz_sign", lambda student, rev: True),              # dz = dh (n - h)
    ("last_word_twice", lambda student, rev: True),      # the last word's weight gradient counted again
    ("student_writes_frozen", lambda student, rev: student),   # student forcing writes (and feeds) every step's logit
    ("ii_jj_swapped", lambda student, rev: student and rev),   # the write test on jj = N-1-ii instead of ii
    # step N - 1's weight and bias gradient sums without the last two words (the carry unchanged): a short or empty
    # last partial of the contraction
    ("tail_samples_dropped", lambda student, rev: True),
)


def param_names(layers):
    names = []
    for l in range(layers):
        names += [f"rnn.{nm}_l{l}" for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return names + ["linear.weight", "linear.bias"]


def writes_of(N, info, student, rev=False, mutation=None):
    w = np.ones(N, bool)
    if student and mutation != "student_writes_frozen":
        w[:] = False
        idx = np.asarray(info, np.int64)
        w[(N - 1 - idx) if (mutation == "ii_jj_swapped" and rev) else idx] = True
    return w


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _encode(fed, onehot):
    """The fed value as the layer-0 input columns: raw, or get_onehot's pair (rnn_all.py:258-260: -1 and 0 -> column 0)."""
    if not onehot:
        return fed[:, None]
    idx = (0.5 + 0.5 * fed).astype(np.int64)
    return np.stack([1.0 - idx, idx.astype(np.float64)], 1)


def forward64(sd, y, layers, onehot, writes, bits=None, mutation=None):
    """decoded (B, N), bits (B, N) and the cache for backward64.  bits given: forced along it (teacher forcing: gt in the
    step frame; or a kernel's returned path).  bits None: student forcing, each step fed the sign of decoded."""
    W = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    y = np.asarray(y, np.float64)
    B, N = y.shape
    F = W["rnn.weight_hh_l0"].shape[1]
    h = [np.zeros((B, F)) for _ in range(layers)]
    decoded = np.ones((B, N))
    path = np.zeros((B, N)) if bits is None else np.asarray(bits, np.float64)
    cache = []
    fed = np.ones(B)
    for ii in range(N):
        x = np.concatenate([y, _encode(fed, onehot)], 1)
        step = []
        inp = x
        for l in range(layers):
            Wih, Whh = W[f"rnn.weight_ih_l{l}"], W[f"rnn.weight_hh_l{l}"]
            bih, bhh = W[f"rnn.bias_ih_l{l}"], W[f"rnn.bias_hh_l{l}"]
            gi = inp @ Wih.T + bih
            gh = h[l] @ Whh.T + bhh
            r = _sig(gi[:, :F] + gh[:, :F])
            z = _sig(gi[:, F:2 * F] + gh[:, F:2 * F])
            ahn = gh[:, 2 * F:]
            if mutation == "bhn_outside":
                ahn = ahn - bhh[2 * F:]
                n = np.tanh(gi[:, 2 * F:] + r * ahn + bhh[2 * F:])
            else:
                n = np.tanh(gi[:, 2 * F:] + r * ahn)
            hn = (h[l] - n) * z + n
            step.append(dict(inp=inp, hp=h[l], r=r, z=z, n=n, ahn=ahn, h=hn))
            h[l] = hn
            inp = hn
        out = h[-1] @ W["linear.weight"].reshape(-1) + W["linear.bias"].reshape(())
        if writes[ii]:
            decoded[:, ii] = out
        if bits is None:
            path[:, ii] = np.sign(decoded[:, ii])
        fed = path[:, ii]
        cache.append(step)
    return decoded, path, dict(cache=cache, W=W, layers=layers, F=F, writes=np.asarray(writes, bool))


def backward64(cx, gout, mutation=None):
    """Gradients (float64, by state-dict name) of sum(gout * decoded): gout (B, N) in the step frame."""
    W, layers, F, cache = cx["W"], cx["layers"], cx["F"], cx["cache"]
    gout = np.asarray(gout, np.float64) * cx["writes"][None, :]   # an unwritten step is the constant 1.0
    B, N = gout.shape
    g = {k: np.zeros_like(v) for k, v in W.items()}
    wrow = np.ones(B)
    if mutation == "last_word_twice":
        wrow[-1] = 2.0
    dh = [np.zeros((B, F)) for _ in range(layers)]
    wl = W["linear.weight"].reshape(-1)
    for ii in range(N - 1, -1, -1):
        go = gout[:, ii]
        if mutation == "tail_samples_dropped":
            wrow = np.ones(B)
            if ii == N - 1:
                wrow[-2:] = 0.0
        g["linear.weight"] += ((go * wrow) @ cache[ii][-1]["h"]).reshape(g["linear.weight"].shape)
        g["linear.bias"] += (go * wrow).sum()
        dh[-1] = dh[-1] + go[:, None] * wl[None, :]
        for l in range(layers - 1, -1, -1):
            c = cache[ii][l]
            d = dh[l]
            dn = d * (1.0 - c["z"])
            dz = d * ((c["n"] - c["hp"]) if mutation == "dz_sign" else (c["hp"] - c["n"]))
            carry = np.zeros_like(d) if mutation == "no_carry" else d * c["z"]
            dan = dn * (1.0 - c["n"] ** 2)
            dahn = dan if mutation == "dahn_no_r" else dan * c["r"]
            dar = dan * c["ahn"] * c["r"] * (1.0 - c["r"])
            daz = dz * c["z"] * (1.0 - c["z"])
            d_ih = np.concatenate([dar, daz, dan], 1)
            d_hh = np.concatenate([dar, daz, dahn], 1)
            g[f"rnn.weight_ih_l{l}"] += (d_ih * wrow[:, None]).T @ c["inp"]
            g[f"rnn.weight_hh_l{l}"] += (d_hh * wrow[:, None]).T @ c["hp"]
            g[f"rnn.bias_ih_l{l}"] += (d_ih * wrow[:, None]).sum(0)
            g[f"rnn.bias_hh_l{l}"] += (d_hh * wrow[:, None]).sum(0)
            dh[l] = carry + d_hh @ W[f"rnn.weight_hh_l{l}"]
            if l > 0:
                dh[l - 1] = dh[l - 1] + d_ih @ W[f"rnn.weight_ih_l{l}"]
    return g


def train64(sd, y, gt_step, layers, onehot, info, student, rev, gout_step, bits=None, mutation=None):
    """decoded, bits, grads in the step frame.  Teacher forcing is forced along gt_step; student forcing feeds itself
    unless `bits` forces a path."""
    N = np.asarray(y).shape[1]
    w = writes_of(N, info, student, rev, mutation)
    path = bits if bits is not None else (None if student else gt_step)
    dec, path, cx = forward64(sd, y, layers, onehot, w, path, mutation)
    return dec, path, backward64(cx, gout_step, mutation)


def rel_err(a, b):
    """||a - b|| / ||b|| in the 2-norm."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def grad_err(got, ref):
    """The largest per-tensor relative error over a case's gradient tensors; every reference tensor must be non-zero."""
    worst = 0.0
    for k, v in ref.items():
        assert np.linalg.norm(np.asarray(v).ravel()) > 0.0, f"gradient {k} is zero"
        worst = max(worst, rel_err(got[k], v))
    return worst


GATES = ("r", "z", "n")


def blocks(grads, F, N):
    """A gradient dict split into the blocks that different parts of the kernels fill: every weight_ih / weight_hh /
    bias_ih / bias_hh by rows into the gates r = [0, F), z = [F, 2F), n = [2F, 3F) (`name.r`, ...); the three row blocks
    of weight_ih_l0 again by columns into the y part [:N] and the fed-bit part [N:] (`name.r.y`, `name.r.bit`, ...);
    linear.* whole."""
    out = {}
    for k, v in grads.items():
        v = np.asarray(v)
        if not k.startswith("rnn."):
            out[k] = v
            continue
        assert v.shape[0] == 3 * F, (k, v.shape)
        for gi, gate in enumerate(GATES):
            blk = v[gi * F:(gi + 1) * F]
            if k.endswith("weight_ih_l0"):
                assert N < blk.shape[1] <= N + 2, (k, v.shape)
                out[f"{k}.{gate}.y"] = blk[:, :N]
                out[f"{k}.{gate}.bit"] = blk[:, N:]
            else:
                out[f"{k}.{gate}"] = blk
    return out


def _shape_of(grads):
    """(F, N) of a gradient dict: weight_hh_l0 is (3F, F); weight_ih_l0 is (3F, N + 1 or N + 2) with N a multiple of 8."""
    F = np.asarray(grads["rnn.weight_hh_l0"]).shape[1]
    return F, np.asarray(grads["rnn.weight_ih_l0"]).shape[1] // 8 * 8


def block_errs(got, ref):
    """Relative 2-norm error of every block (blocks()) of got against ref, by block name."""
    F, N = _shape_of(ref)
    gb, rb = blocks(got, F, N), blocks(ref, F, N)
    assert sorted(gb) == sorted(rb)
    errs = {}
    for k, v in rb.items():
        assert np.linalg.norm(v.ravel()) > 0.0, f"gradient block {k} is zero"
        errs[k] = rel_err(gb[k], v)
    return errs


def grad_err_blocks(got, ref):
    """The largest per-block relative error (blocks()); every reference block must be non-zero.  An error confined
    to one gate, or to the fed-bit columns, is not diluted by the rest of its tensor."""
    return max(block_errs(got, ref).values())


# ---------------------------------------------------------------------------------- torch fp32 autograd (E_ref)
def build_net(F, layers, N, onehot, seed=None, sd=None, device="cpu", g=1.0):
    """The package's RNN_Model: PyTorch-default draws under `seed`, every parameter then times g (g = 4 saturates the
    gates, as forced_helper's decode nets do), or the given state dict."""
    import torch
    from neural_polar_decoder_amd.rnn import RNN_Model
    if seed is not None:
        torch.manual_seed(seed)
    net = RNN_Model("GRU", N + 1 + int(onehot), F, 1, layers, N, 0, 0, "selu", 0.0, False, out_linear_depth=1)
    if g != 1.0:
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(g)
    if sd is not None:
        net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32))) for k, v in sd.items()})
    return net.to(device)


def state_dict_np(net):
    return {k: v.detach().float().cpu().numpy().copy() for k, v in net.state_dict().items()}


def torch_train(net, y, bits, onehot, writes, gout_step):
    """The reference's step loop in torch (net's dtype) forced along `bits`, and autograd's gradients of
    sum(gout * decoded): (decoded, grads by name) as numpy."""
    import torch
    dt = next(net.parameters()).dtype
    net.zero_grad()
    y = torch.as_tensor(np.asarray(y), dtype=dt)
    bits = torch.as_tensor(np.asarray(bits), dtype=dt)
    B, N = y.shape
    hidden = torch.zeros(net.num_rnn_layers, B, net.feature_size, dtype=dt)
    decoded = torch.ones(B, N, dtype=dt)
    fed = torch.ones(B, dtype=dt)
    for ii in range(N):
        if onehot:
            idx = (0.5 + 0.5 * fed).long()
            enc = torch.eye(2, dtype=dt)[idx]
        else:
            enc = fed[:, None]
        out, hidden = net(torch.cat([y, enc], 1).unsqueeze(1), hidden)
        if writes[ii]:
            decoded[:, ii] = out.squeeze(-1)
        fed = bits[:, ii]
    (decoded * torch.as_tensor(np.asarray(gout_step), dtype=dt)).sum().backward()
    grads = {k: p.grad.detach().double().numpy().copy() for k, p in net.named_parameters()}
    return decoded.detach().double().numpy(), grads


def torch_fp32(sd, F, layers, N, onehot, y, bits, writes, gout_step):
    """torch's fp32 step loop and autograd on a case's inputs and path: (decoded, grads by name)."""
    net = build_net(F, layers, N, onehot, sd=sd).float().train()
    return torch_train(net, y, bits, onehot, writes, gout_step)


def e_ref(sd, F, layers, N, onehot, y, bits, writes, gout_step, g64, blockwise=False):
    """E_ref of a case: torch's fp32 autograd on the same inputs against the float64 gradients g64 -- the largest
    per-tensor relative error, or (blockwise) the largest per-block one."""
    _, g32 = torch_fp32(sd, F, layers, N, onehot, y, bits, writes, gout_step)
    return grad_err_blocks(g32, g64) if blockwise else grad_err(g32, g64)


def load_fixture(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    fx = {k: d[k] for k in d.files if not k.startswith(("w.", "teacher.g.", "student.g."))}
    fx["sd"] = {k[2:]: d[k] for k in d.files if k.startswith("w.")}
    for mode in ("teacher", "student"):
        fx[mode + ".g"] = {k[len(mode) + 3:]: d[k] for k in d.files if k.startswith(mode + ".g.")}
    return fx


# ---------------------------------------------------------------------------------- the shape cases
# tests/test_gru_train_shapes.py (CPU: the conditions the cases rest on) and tests/test_gru_train_shapes_gpu.py (the
# kernels).  B = None: 128 CUs + 33 words, one more than a full first grid-stride trip of both recurrence kernels
# (one workgroup per CU, 4 waves x 32 words), ending on a one-word tile; the CPU file takes 256 CUs.
ShapeCase = collections.namedtuple("ShapeCase", "num F layers N B onehot rev student g seed why")
SHAPE_CASES = (
    ShapeCase(1, 32, 1, 8, 33, False, False, True, 1.0, 7201, "minimum length: one k-group of y per lane half"),
    ShapeCase(2, 64, 2, 24, 70, True, True, False, 1.0, 7202, "odd length: 12 floats per lane half"),
    ShapeCase(3, 64, 2, 64, 70, False, True, True, 1.0, 7203, "the quoted shape: two full mask words"),
    ShapeCase(4, 32, 2, 128, 33, True, False, False, 1.0, 7204, "four mask words"),
    ShapeCase(5, 64, 1, 256, 33, True, False, True, 1.0, 7205, "the limit: eight mask words, Din = 258"),
    ShapeCase(6, 64, 2, 256, 70, False, True, True, 1.0, 7206, "the limit on the largest kernel"),
    ShapeCase(7, 64, 2, 64, 1100, True, True, True, 1.0, 7207,
              "split cap: NB = 70,400 (256 partials, chunk 275 -> 276, short last partial); dW_hh K = 69,300 "
              "(chunk 272, empty last partial)"),
    ShapeCase(8, 32, 1, 8, None, True, False, False, 1.0, 7208,
              "second grid-stride trip of both recurrence kernels, ending on a one-word tile and on waves with no "
              "tile; split cap with a chunk of about 1026"),
    ShapeCase(9, 64, 2, 16, 70, True, False, True, 4.0, 7209, "saturated gates"),
    ShapeCase(10, 32, 1, 40, 70, False, True, False, 4.0, 7210, "saturated gates, raw feed"),
)


def shape_id(c):
    return f"case{c.num}-f{c.F}x{c.layers}-n{c.N}-b{c.B or 'cus'}-{'onehot' if c.onehot else 'raw'}-" \
           f"{'rev' if c.rev else 'fwd'}-{'student' if c.student else 'teacher'}-g{c.g:g}"


def shape_batch(c, cus=256):
    return c.B if c.B is not None else 128 * cus + 33


def shape_inputs(c, B):
    """y, gt (position frame) and a random grad_out (position frame) of a shape case at batch B."""
    y, gt = make_words(B, c.N, c.seed)
    gout = np.random.default_rng(c.seed + 1).standard_normal((B, c.N)).astype(np.float32)
    return y, gt, gout


def make_words(B, N, seed):
    """y = +-1 + 0.8 N(0, 1) and a +-1 gt, as the forced-path tests draw them."""
    rng = np.random.default_rng(seed)
    y = (np.where(rng.random((B, N)) < 0.5, -1.0, 1.0) + 0.8 * rng.standard_normal((B, N))).astype(np.float32)
    gt = np.where(rng.random((B, N)) < 0.5, -1.0, 1.0).astype(np.float32)
    return y, gt
