"""Helpers of the forced-path tests (tests/test_forced_path.py, tests/test_forced_path_gpu.py).

When the decision path of RNN_decoder.decode (rnn_all.py:514-561) is given, every step's input is determined, so the
logits of every word at every step can be held to a float64 restatement (oracle.gru_decode_f64(..., path=)) with no
word left out.  An autoregressive decode is verified the same way along the path it REPORTS: float64 forced along the
kernel's decisions, every logit within the bar, every decision the sign of the kernel's own logit -- by induction over
the steps the whole decode, feedback included.

The reference's semantics restated here (pinned by the recorded fixtures, tests/golden/gen_forced.py):
  * reverse_order: step i decodes position N - 1 - i; gt is flipped on entry and decoded flipped back on return
    (rnn_all.py:415-418, :558-561), so gt and decoded are in POSITION order and the logits in STEP order;
  * decoded starts as a raw copy of gt (rnn_all.py:522; ones without gt) and only positions in loss_inds are overwritten
    with sign(logit) (rnn_all.py:530-531, :546-547), so frozen positions keep gt's raw value, whatever it is;
  * the next step is fed sign(decoded) (rnn_all.py:529, :545): get_onehot maps -1 -> column 0, 0 -> column 0
    ((0.5 + 0) .long() = 0), +1 -> column 1; the sign input is the sign itself, 0 included.

CASES holds one entry per instantiated decode kernel (47: gru_decode_kernel 4 shapes x 4 head tilings, gru_decode_bf_kernel
4 shapes x 3 splits, gru16p_kernel 3 splits, gru_wide_kernel 6 shapes, lstm_decode_kernel 3, lstm_wide_kernel 7) at the
smallest code length its route allows, on ragged batches.  Each net is RNN_Model's PyTorch-default draw under its seed
with EVERY parameter times a scale g, so that gates saturate and a dropped product moves the logits far above the bars
(tests/test_forced_path.py holds the conditions on g: the reference's own fp32 arithmetic within bar / 4 of float64,
every MUTATIONS entry at least 10 bars away).
"""
import collections
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FROZEN_VALUES = (-1.0, 1.0, 0.0, -0.3, 2.5)  # genie mode: what gt holds at frozen positions
YH0_HIDDEN, YH0_DEPTH, YH0_ACT = 48, 2, "tanh"  # the y-MLP of the y_h0 cases: Linear(N, 48), tanh, Linear(48, layers F), tanh
LN_EPS = 1e-5
FIXTURES = ("forced_gru_f32_l1_n16_rev", "forced_gru_f64_l2_n32_onehot", "forced_lstm_f32_l2_n16_rev")

# family: the kernel the case runs on; head: None (Linear(F, 1)), "ln" (--use_layernorm) or (out_linear_depth, width);
# bar: the project's logit tolerance of that family / precision (None: plain bf16 has none)
# ys: a further scale on the y columns of rnn.weight_ih_l0 (LONG_CASES; 1.0: none)
Case = collections.namedtuple("Case", "id family cell F layers N B onehot rev precision head yh0 g seed bar ys",
                              defaults=(1.0,))


def bar_of(family, precision):
    if precision == "bf16":
        return None
    if precision == "bf16x3":
        return 2e-3
    return 5e-5 if family == "lstm_wide_kernel" else 2e-5


# scale g per (kind of case); the suggestion is 4, the conditions of tests/test_forced_path.py decide.  With g on every
# parameter the logit grows as g^(1 + head layers): the LayerNorm head (gamma and the Linear both scaled, LayerNorm's
# output of unit variance whatever the state) and the deep heads take a smaller g to keep E_ref within bar / 4.
G_DEFAULT = 4.0
G_LN = 2.0
G_HEAD = {2: 2.5, 3: 2.0}
G_BF16X3 = 4.0
G_YH0 = 3.0


def _cases():
    out = []
    count = collections.Counter()

    def add(family, cell, F, layers, N, precision="fp32", head=None, yh0=False, tag="", g=None):
        i = count[family]
        count[family] += 1
        onehot, rev = i % 2 == 0, (i // 2) % 2 == 1
        B = 40 if F == 512 else 70
        if g is None:
            g = (G_YH0 if yh0 else G_LN if head == "ln" else G_HEAD[head[0]] if head else
                 G_BF16X3 if precision == "bf16x3" else G_DEFAULT)
        cid = f"{family.replace('_kernel', '')}-f{F}x{layers}" + (f"-{precision}" if precision != "fp32" else "") + tag
        out.append(Case(cid, family, cell, F, layers, N, B, onehot, rev, precision, head, yh0, float(g), 4100 + len(out),
                        bar_of(family, precision)))

    heads = [(None, ""), ("ln", "-ln"), ((2, 24), "-d2h24"), ((3, 48), "-d3h48"), ((2, 128), "-d2h128")]
    narrow = [(32, 1), (32, 2), (64, 1), (64, 2)]
    for F, L in narrow:
        for head, tag in heads:
            add("gru_decode_kernel", "GRU", F, L, 16, head=head, tag=tag)
    for F, L in [(64, 1), (32, 2), (32, 1)]:
        add("lstm_decode_kernel", "LSTM", F, L, 16)
    for F, L in narrow:
        for p in ("bf16x3", "bf16", "fp16x3"):
            add("gru_decode_bf_kernel", "GRU", F, L, 16, precision=p)
    for p in ("bf16x3", "bf16", "fp16x3"):
        add("gru16p_kernel", "GRU", 64, 2, 32, precision=p)
    wide = [(128, 1), (128, 2), (256, 1), (256, 2), (512, 1), (512, 2)]
    for F, L in wide:
        add("gru_wide_kernel", "GRU", F, L, 16)
    for F, L in wide + [(64, 2)]:
        add("lstm_wide_kernel", "LSTM", F, L, 16)
    add("gru_decode_kernel", "GRU", 64, 2, 16, yh0=True, tag="-yh0")
    add("gru_wide_kernel", "GRU", 128, 1, 16, yh0=True, tag="-yh0")
    add("lstm_decode_kernel", "LSTM", 32, 2, 16, yh0=True, tag="-yh0")
    add("lstm_wide_kernel", "LSTM", 64, 2, 16, yh0=True, tag="-yh0")
    add("gru16p_kernel", "GRU", 64, 2, 32, precision="fp16x3", yh0=True, tag="-yh0")
    return out


CASES = _cases()
CASE_BY_ID = {c.id: c for c in CASES}
FAMILIES = ("gru_decode_kernel", "gru_decode_bf_kernel", "gru16p_kernel", "gru_wide_kernel", "lstm_decode_kernel",
            "lstm_wide_kernel")
# one case per family for the negative control, B = 1 and rows-past-B tests: the first with a logit bar that is not bf16x3
# (the control must break the bar by a wide factor on the fp32-class bar, the tightest the family has)
FAMILY_CASE = {f: next(c for c in CASES if c.family == f and c.bar == bar_of(f, "fp32") and not c.yh0 and c.head is None)
               for f in FAMILIES}
# the cases whose genie decode also runs with loss_inds = every other position (not the information set)
ALTERNATE_LOSS = ("gru_decode-f64x2", "lstm_decode-f32x2")


# ---- the long and odd lengths: N up to 256 (the interface's limit), lengths that are no power of two, N = 248 where
# F = 512 x 2 layers fills the LDS exactly.  What depends on N in the kernels: the k-steps / K blocks of the y projection,
# the LDS copy of the tile's words, gru16p_kernel's per-step table, the lane-half split, reverse order, and rounding
# that builds up over 256 recurrent steps.  A table of its own: test_case_table_reaches_every_decode_instantiation counts
# CASES.  B = 70 (24 where F = 512).
# A fixed g = 4 does not satisfy the conditions of tests/test_forced_path.py at N = 256: the y projection's variance grows
# with N (PyTorch draws weight_ih_l0 by the hidden size, not by fan-in), the gates saturate, and E_ref leaves bar / 4 (GRU
# 64x2: 1.2e-5 against 5e-6); on the LSTMs lowering g alone leaves no window before max |logit| falls below 1.  So a
# case may scale the y columns of rnn.weight_ih_l0 by ys = sqrt(16 / N) (YS: the projection's variance of N = 16), and
# each row's (g, ys) is the choice, from g in {4, 3.5, 3.25, 3, 2.6, 2.5} and ys in {1, YS}, that the CPU conditions
# accept with E_ref well inside bar / 4 -- measured on the CPU with the functions of this file, never on a kernel:
#   (family, cell, F, layers, N, precision, yh0, g, ys)                              # E_ref forced / genie, max |logit|
YS = "sqrt(16 / N)"
LONG_ROWS = [
    ("gru_decode_kernel", "GRU", 64, 2, 256, "fp32", False, 3.0, YS),                # 2.1e-6 / 2.0e-6, 3.20
    ("gru_decode_kernel", "GRU", 32, 1, 256, "fp32", False, 3.0, YS),                # 1.5e-6 / 1.4e-6, 4.53
    ("gru_decode_kernel", "GRU", 64, 1, 24, "fp32", False, 4.0, 1.0),                # 1.3e-6 / 1.5e-6, 4.20
    ("gru_decode_bf_kernel", "GRU", 32, 2, 256, "fp16x3", False, 2.5, YS),           # 1.5e-6 / 1.1e-6, 2.24
    ("gru_decode_bf_kernel", "GRU", 32, 2, 256, "bf16x3", False, 4.0, 1.0),          # 2.5e-5 / 1.1e-5, 4.20 (bar 2e-3)
    ("gru_decode_bf_kernel", "GRU", 64, 1, 256, "fp16x3", False, 3.0, YS),           # 1.3e-6 / 1.2e-6, 2.53
    ("gru_decode_bf_kernel", "GRU", 64, 1, 256, "bf16x3", False, 4.0, 1.0),          # 5.9e-6 / 6.6e-6, 5.02 (bar 2e-3)
    ("gru_decode_bf_kernel", "GRU", 32, 1, 48, "fp16x3", False, 4.0, 1.0),           # 2.8e-6 / 2.3e-6, 4.31
    ("gru16p_kernel", "GRU", 64, 2, 256, "fp16x3", False, 3.0, YS),                  # 2.0e-6 / 2.0e-6, 2.99
    ("gru16p_kernel", "GRU", 64, 2, 256, "bf16x3", False, 4.0, 1.0),                 # 1.4e-5 / 1.4e-5, 6.34 (bar 2e-3)
    ("gru16p_kernel", "GRU", 64, 2, 96, "fp16x3", False, 4.0, 1.0),                  # 3.4e-6 / 3.5e-6, 4.17 (nkb = 3)
    ("gru16p_kernel", "GRU", 64, 2, 160, "fp16x3", False, 3.0, YS),                  # 1.6e-6 / 1.5e-6, 3.12 (nkb = 5)
    ("gru16p_kernel", "GRU", 64, 2, 256, "fp16x3", True, 4.0, 1.0),                  # 3.3e-6 / 3.5e-6, 3.87 (y_h0)
    ("gru_wide_kernel", "GRU", 128, 2, 256, "fp32", False, 3.0, YS),                 # 1.6e-6 / 1.9e-6, 3.41
    ("gru_wide_kernel", "GRU", 512, 1, 256, "fp32", False, 4.0, 1.0),                # 2.7e-6 / 2.7e-6, 2.86
    ("gru_wide_kernel", "GRU", 256, 1, 40, "fp32", False, 4.0, 1.0),                 # 1.7e-6 / 1.8e-6, 3.75
    ("gru_wide_kernel", "GRU", 512, 2, 248, "fp32", False, 4.0, 1.0),                # 3.8e-6 / 3.4e-6, 6.29 (LDS full)
    ("lstm_decode_kernel", "LSTM", 32, 2, 256, "fp32", False, 2.6, YS),              # 1.8e-6 / 2.4e-6, 1.05
    ("lstm_decode_kernel", "LSTM", 64, 1, 256, "fp32", False, 2.5, YS),              # 6.9e-7 / 7.3e-7, 1.16
    ("lstm_wide_kernel", "LSTM", 256, 2, 256, "fp32", False, 3.25, YS),              # 1.3e-6 / 1.7e-6, 1.17 (bar 5e-5)
    ("lstm_wide_kernel", "LSTM", 512, 2, 248, "fp32", False, 3.5, YS),               # 2.4e-6 / 2.4e-6, 1.45 (LDS full)
]


def _long_cases():
    out = []
    count = collections.Counter()
    for family, cell, F, layers, N, precision, yh0, g, ys in LONG_ROWS:
        i = count[family]
        count[family] += 1
        # (onehot, reverse_order) = (1, 0), (0, 1), (1, 1), (0, 0), (1, 0): both values of both in every family
        onehot, rev = i % 2 == 0, ((i + 1) // 2) % 2 == 1
        cid = (f"{family.replace('_kernel', '')}-f{F}x{layers}" + (f"-{precision}" if precision != "fp32" else "") +
               ("-yh0" if yh0 else "") + f"-n{N}")
        out.append(Case(cid, family, cell, F, layers, N, 24 if F == 512 else 70, onehot, rev, precision, None, yh0,
                        float(g), 4200 + len(out), bar_of(family, precision),
                        (16.0 / N) ** 0.5 if ys == YS else float(ys)))
    return out


LONG_CASES = _long_cases()
# one long case per family for the negative control, B = 1 and rows-past-B tests, chosen as FAMILY_CASE is (B = 70)
LONG_FAMILY_CASE = {f: next(c for c in LONG_CASES
                            if c.family == f and c.bar == bar_of(f, "fp32") and not c.yh0 and c.B == 70) for f in FAMILIES}
CASE_BY_ID.update({c.id: c for c in LONG_CASES})


def info_set(N):
    """The Polar(N, N / 2) information set of the reference (tests/golden/codes.npz, from rnn_all.get_code); where N is
    not a power of two (no code of the reference has that length), a seeded random half of the positions."""
    if N & (N - 1):
        return np.sort(np.random.default_rng(7000 + N).permutation(N)[:N // 2]).astype(np.int64)
    d = np.load(os.path.join(GOLDEN, "codes.npz"))
    return np.asarray(d[f"polar_polar_{N}_{N // 2}_{N // 2}"], np.int64)


def build_net(case, device="cpu", g=None):
    """The case's net: RNN_Model under torch.manual_seed(case.seed), LayerNorm's gamma / beta drawn away from (1, 0),
    then every parameter times g (default case.g), then the y columns of rnn.weight_ih_l0 times case.ys."""
    import torch
    from neural_polar_decoder_amd.rnn import RNN_Model
    torch.manual_seed(case.seed)
    depth, width = case.head if isinstance(case.head, tuple) else (1, 0)
    din = (0 if case.yh0 else case.N) + 1 + int(case.onehot)
    net = RNN_Model(case.cell, din, case.F, 1, case.layers, case.N, YH0_HIDDEN if case.yh0 else width,
                    YH0_DEPTH if case.yh0 else 0, YH0_ACT if case.yh0 else "selu", 0.0, False, out_linear_depth=depth,
                    use_layernorm=case.head == "ln")
    with torch.no_grad():
        if case.head == "ln":
            net.layernorm.weight.uniform_(0.5, 1.5)
            net.layernorm.bias.uniform_(-0.5, 0.5)
        for p in net.parameters():
            p.mul_(case.g if g is None else float(g))
        if case.ys != 1.0:
            assert not case.yh0  # y enters through the y-MLP there, whose Linear(N, .) is drawn by fan-in already
            net.rnn.weight_ih_l0[:, :case.N].mul_(case.ys)
    return net.to(device).eval()


def state_dict_np(net):
    return {k: v.detach().float().cpu().numpy().copy() for k, v in net.state_dict().items()}


def load_np(net, sd):
    import torch
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return net


def make_inputs(case, mode, B=None, alternate=False):
    """(y, gt, loss_inds) of a decode.  mode "forced": gt random +-1, loss_inds [] (every step forced); "genie": loss_inds
    the information set (alternate: every other position) and gt +-1 there, one of FROZEN_VALUES elsewhere; "plain":
    gt None, loss_inds the information set.  y = +-1 + 0.8 N(0, 1), the same words in every mode."""
    B = case.B if B is None else B
    rng = np.random.default_rng(case.seed)
    y = (np.where(rng.random((case.B, case.N)) < 0.5, -1.0, 1.0) + 0.8 * rng.standard_normal((case.B, case.N)))
    y = np.ascontiguousarray(y[case.B - B:], np.float32)  # B < case.B: the last rows
    gt = np.where(rng.random((B, case.N)) < 0.5, -1.0, 1.0).astype(np.float32)
    info = np.arange(1, case.N, 2, dtype=np.int64) if alternate else info_set(case.N)
    if mode == "forced":
        return y, gt, np.zeros(0, np.int64)
    if mode == "plain":
        return y, None, info
    assert mode == "genie"
    frozen = np.setdiff1d(np.arange(case.N), info)
    gt[:, frozen] = np.asarray(FROZEN_VALUES, np.float32)[rng.integers(0, len(FROZEN_VALUES), (B, frozen.size))]
    return y, gt, info


def step_path(decoded, rev):
    """sign of a decoded matrix (position order) in step order: under reverse_order step i is position N - 1 - i.  This is
    what gru_decode_f64's path takes (it feeds the value raw), and what the reference feeds back."""
    d = np.asarray(decoded, np.float64)
    return np.sign(d[:, ::-1] if rev else d)


def f64_forced(case, sd, y, path):
    """float64 logits by step (B, N) of the case's net, forced along path (B, N) of signs in step order."""
    from oracle import oracle as O
    h0x = O.ymlp_f64(y, sd, YH0_ACT, YH0_DEPTH) if case.yh0 else None
    return O.gru_decode_f64(y, sd, case.N, case.F, case.layers, [], onehot=case.onehot, path=path, h0x=h0x,
                            rev=case.rev, cell=case.cell, ln_eps=LN_EPS if case.head == "ln" else None)[1]


def ref32_decode(net, case, y, gt=None, loss_inds=(), path=None):
    """The reference's test loop (rnn_all.py:516-561: :532-547 for y_input, :523-531 for y_h0) in torch fp32 on the CPU,
    one net(...) call per step -> (decoded (B, N) in position order, logits (B, N) by step).  path (signs, step order):
    forced along it instead of along its own decoded."""
    import torch
    from neural_polar_decoder_amd.rnn import get_onehot
    N, B = case.N, y.shape[0]
    onehot_fn = get_onehot if case.onehot else (lambda x: x)
    y = torch.as_tensor(y, dtype=torch.float32)
    order = list(range(N - 1, -1, -1)) if case.rev else list(range(N))
    loss = set(int(i) for i in loss_inds)
    if gt is not None:
        gt = torch.as_tensor(gt, dtype=torch.float32)
        gt = gt.flip(1) if case.rev else gt
    forced = None if path is None else torch.as_tensor(np.ascontiguousarray(path), dtype=torch.float32)
    lg = torch.empty(B, N)
    with torch.no_grad():
        decoded = torch.ones(B, N) if gt is None else gt.clone()
        if case.yh0:
            hidden = net.get_h0(y)
        else:
            hidden = torch.zeros(net.num_rnn_layers, B, net.feature_size)
            hidden = (hidden, hidden) if net.rnn_type == "LSTM" else hidden
        for ii, jj in enumerate(order):
            prev = torch.ones(B) if ii == 0 else (decoded[:, ii - 1].sign() if forced is None else forced[:, ii - 1])
            x = onehot_fn(prev).view(B, 1, -1)
            out, hidden = net(x if case.yh0 else torch.cat([y.unsqueeze(1), x], 2), hidden)
            lg[:, ii] = out.squeeze(1)
            if jj in loss:
                decoded[:, ii] = out.squeeze(1).sign()
    return (decoded.flip(1) if case.rev else decoded).numpy(), lg.numpy()


def ref32_forced(net, case, y, path):
    """Logits by step of the reference's loop forced along path.  |ref32_forced - f64_forced|.max() is E_ref, the error of
    the reference's own arithmetic on these inputs."""
    return ref32_decode(net, case, y, path=path)[1]


# ----------------------------------------------------------------------------------------------- mutations
def _zero_col(key_of):
    def fn(sd, case):
        out = dict(sd)
        for key in key_of(case):
            if key not in sd:
                return None
            w = sd[key].copy()
            w[:, case.F - 1] = 0.0
            out[key] = w
        return out
    return fn


def _swap_cols(a_of, b_of):
    def fn(sd, case):
        a, b = a_of(case), b_of(case)
        if a is None:
            return None
        w = sd["rnn.weight_ih_l0"].copy()
        w[:, [a, b]] = w[:, [b, a]]
        return {**sd, "rnn.weight_ih_l0": w}
    return fn


def _bhn_outside(sd, case):
    if case.cell != "GRU":
        return None
    out = dict(sd)
    F = case.F
    for l in range(case.layers):
        bi, bh = sd[f"rnn.bias_ih_l{l}"].copy(), sd[f"rnn.bias_hh_l{l}"].copy()
        bi[2 * F:] += bh[2 * F:]
        bh[2 * F:] = 0.0
        out[f"rnn.bias_ih_l{l}"], out[f"rnn.bias_hh_l{l}"] = bi, bh
    return out


def _xcol(case):  # first column of weight_ih_l0 after y
    return 0 if case.yh0 else case.N


# typical kernel faults restated as weight edits: fn(state dict, case) -> the mutated state dict, or None where the edit
# does not apply to the case.  A dropped last k element of each product, the lane-half boundary of the y projection,
# the one-hot columns taken the wrong way round, b_hn outside the r product.
MUTATIONS = {
    "whh_l0_last_col": _zero_col(lambda c: ["rnn.weight_hh_l0"]),
    "whh_l1_last_col": _zero_col(lambda c: ["rnn.weight_hh_l1"]),
    "wih_l1_last_col": _zero_col(lambda c: ["rnn.weight_ih_l1"]),
    "head_last_col": _zero_col(lambda c: ["linear.weight" if not isinstance(c.head, tuple) else "linear.0.weight"]),
    "y_cols_swapped": _swap_cols(lambda c: None if c.yh0 else c.N // 2 - 1, lambda c: c.N // 2),
    "onehot_cols_swapped": _swap_cols(lambda c: _xcol(c) if c.onehot else None, lambda c: _xcol(c) + 1),
    "bhn_outside_r": _bhn_outside,
}
NEGATIVE_CONTROL = "whh_l0_last_col"

# (case id, mutation) pairs that cannot reach 10 bars on half the words at any g that keeps E_ref <= bar / 4, with the
# reason; tests/test_forced_path.py requires every other pair to reach it and every pair listed here NOT to (so that
# the table cannot go stale).
MUTATION_EXCEPTIONS = {}


def mutation_reach(l64, l64_mut):
    """Per word, the largest move of the float64 logits over the steps."""
    return np.abs(l64_mut - l64).max(1)


# ----------------------------------------------------------------------------------------------- the check
def check_forced(kernel_logits, kernel_decoded, gt, loss_inds, l64, bar, rev=False):
    """The assertions of a decode verified along its own reported path, over ALL words and steps: logits finite and
    (bar given) within bar of the float64 logits l64 forced along step_path(kernel_decoded); decoded at loss positions
    exactly sign(kernel logit); decoded elsewhere bitwise gt (1.0 without gt).  Returns max |logit - float64|."""
    lg = np.asarray(kernel_logits)
    dec = np.asarray(kernel_decoded, np.float32)
    B, N = dec.shape
    assert lg.shape == (B, N) and l64.shape == (B, N)
    assert np.all(np.isfinite(lg)), "a logit is not finite"
    err = np.abs(lg.astype(np.float64) - l64)
    if bar is not None:
        w, s = np.unravel_index(err.argmax(), err.shape)
        assert err.max() < bar, f"logit off float64 by {err.max():.3e} (bar {bar:.1e}) at word {w} step {s}"
    loss = np.zeros(N, bool)
    loss[np.asarray(loss_inds, np.int64)] = True
    lg_pos = lg[:, ::-1] if rev else lg  # step i is position N - 1 - i
    assert np.array_equal(dec[:, loss], np.sign(lg_pos[:, loss]).astype(np.float32)), \
        "a decision is not the sign of the kernel's own logit"
    want = np.ones((B, N), np.float32) if gt is None else np.ascontiguousarray(gt, np.float32)
    assert np.array_equal(dec[:, ~loss].view(np.uint32), want[:, ~loss].view(np.uint32)), \
        "a position outside loss_inds is not the raw gt value"
    return float(err.max())


def load_fixture(name):
    """(Case, fixture, state dict) of a fixture recorded from the reference (tests/golden/gen_forced.py)."""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    cell = bytes(d["cell"]).decode()
    F, layers, N = int(d["F"]), int(d["layers"]), int(d["N"])
    family = "lstm_decode_kernel" if cell == "LSTM" else "gru_decode_kernel"
    case = Case(name, family, cell, F, layers, N, int(d["y"].shape[0]), bool(d["onehot"]), bool(d["rev"]), "fp32", None,
                False, float(d["g"]), int(d["seed"]), bar_of(family, "fp32"))
    if "w.linear.weight" in d.files:
        sd = {k[2:]: np.asarray(d[k]) for k in d.files if k.startswith("w.")}
    else:  # past the fixture size limit: the same draws from the stored seed, scaled by the stored g
        sd = state_dict_np(build_net(case))
    assert weights_digest(sd) == bytes(d["w_digest"]).decode(), "the fixture's net is not the one it was recorded with"
    return case, d, sd


def weights_digest(sd):
    """sha256 over a state dict's arrays in sorted key order (as tests/conftest.py)."""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], np.float32).tobytes())
    return h.hexdigest()
