"""CRISP GRU training at long codes, large batches and saturated gates, CPU side: the conditions that the GPU cases of
tests/test_gru_train_shapes_gpu.py rest on, kept by the references alone (the float64 restatement of
tests/train_helper.py and torch's fp32 autograd), for every case of train_helper.SHAPE_CASES.

  - every block (train_helper.blocks) of the float64 gradient is non-zero, so a per-block relative error exists
  - every logit at a written step differs from 1.0, the constant of the unwritten steps
  - torch's fp32 logits are within LOGIT_BAR / 4 of float64: the logit bar leaves a correct fp32 kernel room, at
    N = 256 and with saturated gates (g = 4) too
  - the gradient bar GRAD_FACTOR x E_ref, whole-tensor and per block, each against its own E_ref, tells every mutation
    of train_helper.MUTATIONS from rounding by >= 10 x (the cases with B <= 1100; case 8 is exempt only to keep this
    file short)

Student forcing here feeds the restatement's own float64 path; the GPU file forces the restatement along the kernel's.
Case 8's batch depends on the GPU's CU count; here it is taken at 256 CUs.
"""
import numpy as np
import pytest

import forced_helper as H
import train_helper as T


def _step(a, rev):
    return np.ascontiguousarray(a[:, ::-1]) if rev else a


@pytest.fixture(scope="module", params=T.SHAPE_CASES, ids=T.shape_id)
def ref(request):
    """One case's float64 and torch fp32 results, computed once and left unchanged."""
    c = request.param
    B = T.shape_batch(c)
    sd = T.state_dict_np(T.build_net(c.F, c.layers, c.N, c.onehot, seed=c.seed, g=c.g))
    info = H.info_set(c.N)
    y, gt, gout = T.shape_inputs(c, B)
    gt_s, gout_s = _step(gt, c.rev), _step(gout, c.rev)
    dec64, bits, g64 = T.train64(sd, y, gt_s, c.layers, c.onehot, info, c.student, c.rev, gout_s)
    w = T.writes_of(c.N, info, c.student)
    dec32, g32 = T.torch_fp32(sd, c.F, c.layers, c.N, c.onehot, y, bits, w, gout_s)
    return dict(c=c, B=B, sd=sd, info=info, y=y, gt_s=gt_s, gout_s=gout_s, dec64=dec64, bits=bits, g64=g64, w=w,
                dec32=dec32, g32=g32)


def test_reference_conditions(ref):
    c, g64, w = ref["c"], ref["g64"], ref["w"]
    for k, v in T.blocks(g64, c.F, c.N).items():
        assert np.linalg.norm(v.ravel()) > 0.0, f"float64 gradient block {k} is zero"
    assert w.any() and w[c.N - 1], "the last step writes a logit in every case"
    assert np.all(ref["dec64"][:, w] != 1.0) and np.all(ref["dec64"][:, ~w] == 1.0)
    lerr = float(np.abs(ref["dec32"] - ref["dec64"]).max())
    eref, eref_b = T.grad_err(ref["g32"], g64), T.grad_err_blocks(ref["g32"], g64)
    be = T.block_errs(ref["g32"], g64)
    print(f"{T.shape_id(c)} (B = {ref['B']}): torch fp32 logit err {lerr:.2e} (bar / 4 = {T.LOGIT_BAR / 4:.1e}); "
          f"E_ref {eref:.2e}, blockwise E_ref {eref_b:.2e} at {max(be, key=be.get)}; "
          f"max |logit| {np.abs(ref['dec64'][:, w]).max():.1f}")
    assert lerr <= T.LOGIT_BAR / 4
    assert eref_b >= eref * (1 - 1e-12), "a tensor's error is no larger than its worst block's"


def test_saturated_cases_saturate(ref):
    """g = 4 is there to push the gates to the ends of their range, where 1 - z, r (1 - r) and 1 - n^2 cancel: some r
    and some z within 1e-3 of 0 and of 1 and some |n| within 1e-3 of 1, that is |pre-activation| > 6.9 for the
    sigmoids and > 3.8 for tanh, against <~ 2 in a PyTorch-default draw."""
    c = ref["c"]
    if c.g == 1.0:
        return
    w = T.writes_of(c.N, ref["info"], c.student)
    _, _, cx = T.forward64(ref["sd"], ref["y"], c.layers, c.onehot, w, ref["bits"])
    z = np.stack([s[l]["z"] for s in cx["cache"] for l in range(c.layers)])
    n = np.stack([s[l]["n"] for s in cx["cache"] for l in range(c.layers)])
    r = np.stack([s[l]["r"] for s in cx["cache"] for l in range(c.layers)])
    print(f"{T.shape_id(c)}: z in [{z.min():.1e}, 1 - {1 - z.max():.1e}], r in [{r.min():.1e}, 1 - {1 - r.max():.1e}], "
          f"max |n| = 1 - {1 - np.abs(n).max():.1e}")
    assert z.min() < 1e-3 and z.max() > 1 - 1e-3 and r.min() < 1e-3 and r.max() > 1 - 1e-3
    assert np.abs(n).max() > 1 - 1e-3


def test_mutations_miss_both_bars(ref):
    c, g64 = ref["c"], ref["g64"]
    if ref["B"] > 1100:
        return  # case 8: exempt, to keep the CPU suite short
    bar = T.GRAD_FACTOR * T.grad_err(ref["g32"], g64)
    bar_b = T.GRAD_FACTOR * T.grad_err_blocks(ref["g32"], g64)
    print(f"{T.shape_id(c)}: bar {bar:.2e}, block bar {bar_b:.2e}")
    ran = 0
    for name, applies in T.MUTATIONS:
        if not applies(c.student, c.rev):
            continue
        dec_m, _, g_m = T.train64(ref["sd"], ref["y"], ref["gt_s"], c.layers, c.onehot, ref["info"], c.student, c.rev,
                                  ref["gout_s"], mutation=name)
        derr = T.rel_err(dec_m, ref["dec64"])
        miss, miss_b = max(T.grad_err(g_m, g64), derr), max(T.grad_err_blocks(g_m, g64), derr)
        print(f"  mutation {name}: {miss:.2e} = {miss / bar:.1e} x bar; blocks {miss_b:.2e} = {miss_b / bar_b:.1e} x bar")
        assert miss >= 10.0 * bar, name
        assert miss_b >= 10.0 * bar_b, name
        ran += 1
    assert ran >= 6


def test_blocks_partition_every_tensor():
    """blocks() loses no element and names the bit columns: the blocks' squared norms add up to the tensors'."""
    c = T.SHAPE_CASES[1]
    sd = T.state_dict_np(T.build_net(c.F, c.layers, c.N, c.onehot, seed=c.seed))
    b = T.blocks(sd, c.F, c.N)
    assert np.isclose(sum(float((v.astype(np.float64) ** 2).sum()) for v in b.values()),
                      sum(float((v.astype(np.float64) ** 2).sum()) for v in sd.values()), rtol=1e-12)
    assert b["rnn.weight_ih_l0.z.bit"].shape == (c.F, 2) and b["rnn.weight_ih_l0.n.y"].shape == (c.F, c.N)
    assert np.array_equal(b["rnn.weight_hh_l1.n"], sd["rnn.weight_hh_l1"][2 * c.F:])
    assert np.array_equal(b["rnn.weight_ih_l0.z.bit"], sd["rnn.weight_ih_l0"][c.F:2 * c.F, c.N:])
    assert len(b) == 3 * 4 * c.layers + 3 + 2
    # an error confined to the bit columns of one gate shows in full on the block metric, diluted on the tensor's
    bad = {k: v.copy() for k, v in sd.items()}
    bad["rnn.weight_ih_l0"][c.F:2 * c.F, c.N:] *= 1.01
    assert abs(T.grad_err_blocks(bad, sd) - 0.01) < 1e-6 and T.grad_err(bad, sd) < 0.004


def test_g_scales_every_parameter():
    a = T.state_dict_np(T.build_net(32, 1, 8, True, seed=7299))
    b = T.state_dict_np(T.build_net(32, 1, 8, True, seed=7299, g=4.0))
    assert sorted(a) == sorted(b) and all(np.array_equal(np.float32(4.0) * a[k], b[k]) for k in a)
