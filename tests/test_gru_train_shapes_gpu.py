"""CRISP GRU training on the fused kernels at long codes, large batches and saturated gates, on the MI355X.

The protocol is tests/test_gru_train_gpu.py's: decode(net, True, ..., return_path=True) and a backward with a random
grad_out, held to the float64 restatement (tests/train_helper.py) forced along the kernel's own returned path --
logits within LOGIT_BAR, gradients within GRAD_FACTOR x E_ref on the whole-tensor metric and also on the block metric
(train_helper.blocks: one block per gate of every 3F-row tensor, weight_ih_l0 again by its y and fed-bit columns), each
against its own E_ref, torch's fp32 autograd on the same inputs and path.  tests/test_gru_train_shapes.py holds, on the
CPU, the conditions these cases rest on.

train_helper.SHAPE_CASES says what each case exists for: every mask-word count of N (8 .. 256), the contraction at its
cap of 256 partials with a short and an empty last one, a second grid-stride trip of both recurrence kernels, and nets
scaled by g = 4 so that the gates saturate.  The further tests are the autograd contract: y changed in place, two
forwards before one backward on a shared plan, retain_graph, an expanded grad_out, a side stream.
"""
import numpy as np
import pytest
import torch

import forced_helper as H
import train_helper as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE1, CASE3 = T.SHAPE_CASES[0], T.SHAPE_CASES[2]


def _flip(a, rev):
    return np.ascontiguousarray(a[:, ::-1]) if rev else a


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def setup(c, B=None, seed=None):
    from neural_polar_decoder_amd.rnn import RNN_decoder
    B = T.shape_batch(c, _cus()) if B is None else B
    net = T.build_net(c.F, c.layers, c.N, c.onehot, seed=c.seed if seed is None else seed, device=DEV, g=c.g)
    info = H.info_set(c.N)
    dec = RNN_decoder("y_input", c.N, info, onehot=c.onehot, reverse_order=c.rev)
    y, gt, gout = T.shape_inputs(c, B)
    return net, dec, info, y, gt, gout


def decode(net, dec, c, y, gt, student=None):
    """decode(net, True, ...) on device tensors: (out (position frame, with a grad_fn), bits (step frame))."""
    student = c.student if student is None else student
    return dec.decode(net, True, y, gt, 0.0 if student else 1.0, return_path=True)


def grads_of(net):
    return {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}


def run(net, dec, c, y, gt, gout, student=None):
    """One forward and backward from host arrays: (out (position frame), bits (step frame), grads by name), numpy."""
    net.zero_grad()
    out, bits = decode(net, dec, c, torch.from_numpy(y).to(DEV), torch.from_numpy(gt).to(DEV), student)
    assert out.grad_fn is not None and out.dtype == torch.float32 and out.shape == y.shape
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    return out.detach().cpu().numpy(), bits.cpu().numpy(), grads_of(net)


def same(g1, g2):
    assert sorted(g1) == sorted(g2)
    for k in g1:
        assert np.linalg.norm(g1[k]) > 0 and np.array_equal(g1[k], g2[k]), k


@pytest.mark.parametrize("c", T.SHAPE_CASES, ids=T.shape_id)
def test_forward_and_gradients_against_float64(c):
    net, dec, info, y, gt, gout = setup(c)
    B = y.shape[0]
    if c.B is None:
        assert B > 128 * _cus(), "case 8 needs a second grid-stride trip"
    sd = T.state_dict_np(net)
    out, bits, grads = run(net, dec, c, y, gt, gout)
    out_s, gt_s, gout_s = _flip(out, c.rev), _flip(gt, c.rev), _flip(gout, c.rev)
    w = T.writes_of(c.N, info, c.student)
    assert not np.isnan(out).any() and not np.isnan(bits).any()
    # ---- the path
    if c.student:
        assert np.all(out_s[:, ~w] == 1.0)
        assert np.array_equal(bits[:, w], np.sign(out_s[:, w])) and np.all(bits[:, ~w] == 1.0)
    else:
        assert w.all() and np.array_equal(bits, gt_s)
    # ---- forward and backward against float64 along that path
    dec64, _, g64 = T.train64(sd, y, gt_s, c.layers, c.onehot, info, c.student, c.rev, gout_s, bits=bits)
    lerr = float(np.abs(out_s - dec64).max())
    _, g32 = T.torch_fp32(sd, c.F, c.layers, c.N, c.onehot, y, bits, w, gout_s)
    eref, eref_b = T.grad_err(g32, g64), T.grad_err_blocks(g32, g64)
    errs, berrs = {k: T.rel_err(grads[k], g64[k]) for k in g64}, T.block_errs(grads, g64)
    gerr, gerr_b = T.grad_err(grads, g64), T.grad_err_blocks(grads, g64)
    print(f"{T.shape_id(c)} (B = {B}): logit err {lerr:.2e} (bar {T.LOGIT_BAR:.0e}); grad err {gerr:.2e}, E_ref "
          f"{eref:.2e}, ratio {gerr / eref:.2f}; block err {gerr_b:.2e}, block E_ref {eref_b:.2e}, ratio "
          f"{gerr_b / eref_b:.2f} (bar {T.GRAD_FACTOR:.0f}); worst tensor {max(errs, key=errs.get)}, worst block "
          f"{max(berrs, key=berrs.get)}")
    assert np.isfinite(out).all() and lerr <= T.LOGIT_BAR
    assert sorted(grads) == sorted(g64)
    assert gerr <= T.GRAD_FACTOR * eref, errs
    assert gerr_b <= T.GRAD_FACTOR * eref_b, berrs
    if c.B is None:
        # rows do not depend on the batch: words of the first trip and of the second (the last 33, the one-word tile
        # among them), decoded alone in a batch of 64, are bit-identical
        idx = np.concatenate([np.arange(31), np.arange(B - 33, B)])
        assert idx[31] == 128 * _cus()
        o64, b64 = decode(net, dec, c, torch.from_numpy(y[idx]).to(DEV), torch.from_numpy(gt[idx]).to(DEV))
        assert np.array_equal(o64.detach().cpu().numpy(), out[idx]) and np.array_equal(b64.cpu().numpy(), bits[idx])


def test_y_changed_in_place_before_backward_raises_or_changes_nothing():
    """The backward reads y for dW_ih0's y columns: after y.normal_() it raises (torch's version counter) or returns
    the gradients of the untouched run bit for bit -- never those of another y."""
    c = CASE3
    net, dec, info, y, gt, gout = setup(c)
    _, _, g1 = run(net, dec, c, y, gt, gout)
    net.zero_grad()
    yd = torch.from_numpy(y).to(DEV)
    out, _ = decode(net, dec, c, yd, torch.from_numpy(gt).to(DEV))
    loss = (out * torch.from_numpy(gout).to(DEV)).sum()
    yd.normal_()
    try:
        loss.backward()
    except RuntimeError as e:
        assert "modified by an inplace operation" in str(e)
        return
    same(g1, grads_of(net))


def test_two_forwards_before_one_backward_on_a_shared_plan():
    """Two nets of one shape share a plan, whose images are repacked per call: each net's gradients from one backward
    of both losses are those of the same call made alone, bit for bit."""
    from neural_polar_decoder_amd import rnn
    c = CASE3
    netA, dec, info, yA, gtA, goA = setup(c, B=33)
    netB, _, _, yB, gtB, goB = setup(c, B=70, seed=c.seed + 50)
    assert not np.array_equal(T.state_dict_np(netA)["linear.weight"], T.state_dict_np(netB)["linear.weight"])
    _, _, gA = run(netA, dec, c, yA, gtA, goA)
    _, _, gB = run(netB, dec, c, yB, gtB, goB)
    plans = len(rnn._TRAIN_PLANS)
    netA.zero_grad()
    netB.zero_grad()
    outA, _ = decode(netA, dec, c, torch.from_numpy(yA).to(DEV), torch.from_numpy(gtA).to(DEV))
    outB, _ = decode(netB, dec, c, torch.from_numpy(yB).to(DEV), torch.from_numpy(gtB).to(DEV))
    assert len(rnn._TRAIN_PLANS) == plans, "the two nets share one plan"
    ((outA * torch.from_numpy(goA).to(DEV)).sum() + (outB * torch.from_numpy(goB).to(DEV)).sum()).backward()
    same(gA, grads_of(netA))
    same(gB, grads_of(netB))


def test_second_backward_with_retain_graph_doubles_grad():
    c = CASE1
    net, dec, info, y, gt, gout = setup(c)
    net.zero_grad()
    out, _ = decode(net, dec, c, torch.from_numpy(y).to(DEV), torch.from_numpy(gt).to(DEV))
    loss = (out * torch.from_numpy(gout).to(DEV)).sum()
    loss.backward(retain_graph=True)
    g1 = grads_of(net)
    loss.backward()
    g2 = grads_of(net)
    for k in g1:
        assert np.linalg.norm(g1[k]) > 0 and np.array_equal(g2[k], np.float32(2.0) * g1[k]), k


@pytest.mark.parametrize("c,student", [(CASE1, False), (CASE3, True)], ids=["fwd-teacher", "rev-student"])
def test_expanded_grad_out_equals_explicit_ones(c, student):
    """out.sum().backward() hands the function a stride-0 grad_out (teacher forcing, forward order: straight into the
    kernel's .contiguous(); reverse order: through flip): bit-equal to an explicit torch.ones."""
    net, dec, info, y, gt, _ = setup(c)
    yd, gd = torch.from_numpy(y).to(DEV), torch.from_numpy(gt).to(DEV)
    net.zero_grad()
    out, _ = decode(net, dec, c, yd, gd, student)
    out.backward(torch.ones(out.shape, device=DEV))
    g1 = grads_of(net)
    net.zero_grad()
    out, _ = decode(net, dec, c, yd, gd, student)
    out.sum().backward()
    same(g1, grads_of(net))


def test_side_stream_equals_default_stream():
    c = CASE3
    net, dec, info, y, gt, gout = setup(c)
    o1, b1, g1 = run(net, dec, c, y, gt, gout)
    yd, gd, god = torch.from_numpy(y).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(gout).to(DEV)
    net.zero_grad()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        out, bits = decode(net, dec, c, yd, gd)
        (out * god).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(out.detach().cpu().numpy(), o1) and np.array_equal(bits.cpu().numpy(), b1)
    same(g1, grads_of(net))
