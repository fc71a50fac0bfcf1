"""CRISP GRU training on the fused kernels (npd_gru_train_forward / _backward), on the MI355X.

Every case runs RNN_decoder.decode(net, True, y, gt, tfr, return_path=True) and a backward with a RANDOM grad_out, and
is held to the float64 restatement (tests/train_helper.py) forced along the kernel's own returned path:

  forward   |logit - float64 logit| <= 2e-5 (the project's fp32 GRU bar, forced_helper.bar_of); teacher forcing: bits ==
            gt; student forcing: bits == sign(own logit) at the written steps and +1 elsewhere, where out is exactly 1.0
  backward  every gradient tensor within 16 E_ref of float64 (relative, 2-norm), E_ref = torch's own fp32 autograd on
            the same inputs and path, computed in the test on the CPU (tests/test_gru_train.py says why 16)

Nets are PyTorch-default draws under a seed.  CASES thins the cross product (shape x mode x onehot x order x N x B) the way
forced_helper.CASES does: every kernel instantiation, flag, length and batch size at least once.  N = 40 is no multiple
of 16 and its information mask crosses the 32-bit word; B = 200 spans two workgroups, makes the contraction reduce more
than one partial and ends on a ragged tile; B = 1, 33, 70 end on ragged tiles of one word, one word past a tile, and 6.
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

import forced_helper as H
import train_helper as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

Case = collections.namedtuple("Case", "F layers N B onehot rev student seed")
CASES = [
    Case(32, 1, 16, 1, False, False, False, 7101),
    Case(32, 1, 40, 33, True, True, True, 7102),
    Case(32, 2, 16, 70, True, False, True, 7103),
    Case(32, 2, 40, 200, False, True, False, 7104),
    Case(64, 1, 40, 70, False, True, True, 7105),
    Case(64, 1, 16, 200, True, False, False, 7106),
    Case(64, 2, 16, 33, False, True, False, 7107),
    Case(64, 2, 40, 200, True, False, True, 7108),
    Case(64, 2, 16, 1, True, True, True, 7109),
]
SMALL = CASES[2]


def _id(c):
    return f"f{c.F}x{c.layers}-n{c.N}-b{c.B}-{'onehot' if c.onehot else 'raw'}-{'rev' if c.rev else 'fwd'}-" \
           f"{'student' if c.student else 'teacher'}"


def _flip(a, rev):
    return np.ascontiguousarray(a[:, ::-1]) if rev else a


def setup(c, B=None):
    from neural_polar_decoder_amd.rnn import RNN_decoder
    B = c.B if B is None else B
    net = T.build_net(c.F, c.layers, c.N, c.onehot, seed=c.seed, device=DEV)
    info = H.info_set(c.N)
    dec = RNN_decoder("y_input", c.N, info, onehot=c.onehot, reverse_order=c.rev)
    y, gt = T.make_words(B, c.N, c.seed)
    gout = np.random.default_rng(c.seed + 1).standard_normal((B, c.N)).astype(np.float32)
    return net, dec, info, y, gt, gout


def run(net, dec, c, y, gt, gout):
    """One forward and backward: (out (position frame), bits (step frame), grads by name), numpy."""
    net.zero_grad()
    out, bits = dec.decode(net, True, torch.from_numpy(y).to(DEV), torch.from_numpy(gt).to(DEV),
                           0.0 if c.student else 1.0, return_path=True)
    assert out.grad_fn is not None and out.dtype == torch.float32 and out.shape == y.shape and net.training
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}
    return out.detach().cpu().numpy(), bits.cpu().numpy(), grads


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_forward_and_gradients_against_float64(c):
    net, dec, info, y, gt, gout = setup(c)
    sd = T.state_dict_np(net)
    out, bits, grads = run(net, dec, c, y, gt, gout)
    out_s, gt_s, gout_s = _flip(out, c.rev), _flip(gt, c.rev), _flip(gout, c.rev)
    w = T.writes_of(c.N, info, c.student)
    # ---- the path
    if c.student:
        assert np.all(out_s[:, ~w] == 1.0)
        assert np.array_equal(bits[:, w], np.sign(out_s[:, w])) and np.all(bits[:, ~w] == 1.0)
    else:
        assert w.all() and np.array_equal(bits, gt_s)
    # ---- forward and backward against float64 along that path
    dec64, _, g64 = T.train64(sd, y, gt_s, c.layers, c.onehot, info, c.student, c.rev, gout_s, bits=bits)
    lerr = float(np.abs(out_s - dec64).max())
    eref = T.e_ref(sd, c.F, c.layers, c.N, c.onehot, y, bits, w, gout_s, g64)
    errs = {k: T.rel_err(grads[k], g64[k]) for k in g64}
    gerr = T.grad_err(grads, g64)
    print(f"{_id(c)}: logit err {lerr:.2e} (bar {T.LOGIT_BAR:.0e}); grad err {gerr:.2e}, E_ref {eref:.2e}, "
          f"ratio {gerr / eref:.2f} (bar {T.GRAD_FACTOR:.0f}); worst tensor {max(errs, key=errs.get)}")
    assert np.isfinite(out).all() and lerr <= T.LOGIT_BAR
    assert sorted(grads) == sorted(g64)
    assert gerr <= T.GRAD_FACTOR * eref, errs


def test_identical_calls_return_identical_bits():
    c = CASES[7]  # B = 200: several partial sums
    net, dec, info, y, gt, gout = setup(c)
    o1, b1, g1 = run(net, dec, c, y, gt, gout)
    o2, b2, g2 = run(net, dec, c, y, gt, gout)
    assert np.array_equal(o1, o2) and np.array_equal(b1, b2)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k


def test_student_grad_out_at_unwritten_steps_has_no_effect():
    c = SMALL
    net, dec, info, y, gt, gout = setup(c)
    _, _, g1 = run(net, dec, c, y, gt, gout)
    w = T.writes_of(c.N, info, True)
    g2o = _flip(gout, c.rev).copy()
    g2o[:, ~w] += 3.0
    _, _, g2 = run(net, dec, c, y, gt, _flip(g2o, c.rev))
    for k in g1:
        assert np.linalg.norm(g1[k]) > 0 and np.array_equal(g1[k], g2[k]), k


def test_gradients_accumulate_into_existing_grad():
    c = SMALL
    net, dec, info, y, gt, gout = setup(c)
    _, _, g1 = run(net, dec, c, y, gt, gout)
    net.zero_grad()
    for p in net.parameters():
        p.grad = torch.full_like(p, 0.5)
    out = dec.decode(net, True, torch.from_numpy(y).to(DEV), torch.from_numpy(gt).to(DEV), 0.0)
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    for k, p in net.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy(), np.float32(0.5) + g1[k]), k


def test_rows_past_the_batch_stay_untouched():
    """The C entry point with out / bits buffers of B + 3 rows: the rows past B keep their fill."""
    from neural_polar_decoder_amd import _lib
    from neural_polar_decoder_amd.rnn import _train_params, _train_plan
    c = CASES[1]  # B = 33: one word in the second tile
    net, dec, info, y, gt, _ = setup(c)
    B, N = y.shape
    plan = _train_plan(torch.device(DEV), N, c.F, c.layers, c.onehot)
    flat = torch.cat([p.detach().reshape(-1) for p in _train_params(net)]).contiguous()
    n_saved, n_scratch = plan.workspace(B)
    assert n_saved == N * B * (5 * c.layers * c.F + 3) and n_scratch > N * B * 4 * c.F * c.layers
    saved = torch.empty(n_saved, device=DEV)
    out = torch.full((B + 3, N), -7.0, device=DEV)
    bits = torch.full((B + 3, N), -7.0, device=DEV)
    writes = T.writes_of(N, info, True).astype(np.uint8)
    yd = torch.from_numpy(y).to(DEV)
    _lib.check(_lib.load().npd_gru_train_forward(plan.h, _lib.ptr(flat), _lib.ptr(yd), None,
                                                 writes.ctypes.data_as(ctypes.c_void_p), 1, _lib.ptr(out), _lib.ptr(bits),
                                                 _lib.ptr(saved), B, _lib.stream_of(torch.device(DEV))), "forward")
    torch.cuda.synchronize()
    assert bool((out[B:] == -7.0).all()) and bool((bits[B:] == -7.0).all())
    assert bool((out[:B] != -7.0).all()) and bool((bits[:B].abs() == 1.0).all())
    # argument errors come back as a status, before any device work
    L = _lib.load()
    assert L.npd_gru_train_forward(plan.h, _lib.ptr(flat), _lib.ptr(yd), None, writes.ctypes.data_as(ctypes.c_void_p), 0,
                                   _lib.ptr(out), _lib.ptr(bits), _lib.ptr(saved), B, None) < 0   # teacher without gt
    assert b"gt" in L.npd_last_error()


def test_empty_batch_returns_empty():
    c = SMALL
    net, dec, info, y, gt, _ = setup(c)
    out = dec.decode(net, True, torch.empty(0, c.N, device=DEV), torch.empty(0, c.N, device=DEV), 1.0)
    assert out.shape == (0, c.N) and out.dtype == torch.float32 and out.device.type == "cuda"


def test_next_forward_sees_the_stepped_weights():
    """After optimizer.step() the logits are the restatement's with the UPDATED weights: a stale image fails this."""
    c = CASES[6]
    net, dec, info, y, gt, gout = setup(c)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    out0, _, _ = run(net, dec, c, y, gt, gout)
    opt.step()
    sd = T.state_dict_np(net)
    out1, bits = dec.decode(net, True, torch.from_numpy(y).to(DEV), torch.from_numpy(gt).to(DEV), 1.0, return_path=True)
    out1_s = _flip(out1.detach().cpu().numpy(), c.rev)
    w = T.writes_of(c.N, info, False)
    dec64, _, _ = T.forward64(sd, y, c.layers, c.onehot, w, bits.cpu().numpy())
    assert float(np.abs(out1_s - dec64).max()) <= T.LOGIT_BAR
    assert float(np.abs(out1_s - _flip(out0, c.rev)).max()) > 100 * T.LOGIT_BAR, "the step did not move the logits"


def test_trainer_mult_2_clips_steps_and_checkpoints(tmp_path):
    """neural_polar_decoder_amd.train for 4 steps on Polar(16, 4) with mult = 2 (two backward calls accumulate before
    clip_grad_norm_ and a step); the checkpoint loads through rnn_from_checkpoint and decodes."""
    from neural_polar_decoder_amd import train as TR
    from neural_polar_decoder_amd.datasets import rnn_from_checkpoint
    path = str(tmp_path / "crisp.pt")
    args = TR.parse_args(["--N", "16", "--K", "4", "--rnn_feature_size", "32", "--rnn_depth", "2", "--onehot",
                          "--num_steps", "4", "--batch_size", "256", "--dec_train_snr", "1", "--mult", "2", "--clip", "0.5",
                          "--tfr_max", "0.5", "--teacher_steps", "1", "--lr", "0.01", "--scheduler", "step", "--lr_decay", "2",
                          "--save_path", path, "--print_freq", "0"])
    torch.manual_seed(args.random_seed)
    ref = T.build_net(32, 2, 16, True, device=DEV)
    before = T.state_dict_np(ref)   # the trainer draws its net under the same seed
    net, dec, code, losses = TR.train(args, device=DEV)
    assert len(losses) == 4 and np.isfinite(losses).all()
    after = T.state_dict_np(net)
    assert all(not np.array_equal(before[k], after[k]) for k in before), "a parameter never moved"
    net2, dec2, code2 = rnn_from_checkpoint(path, device=DEV)
    assert all(np.array_equal(T.state_dict_np(net2)[k], after[k]) for k in after)
    _, _, y = code2.mc_generate(64, 1.0, seed=3, device=torch.device(DEV))
    d = dec2.decode(net2, False, y)
    assert d.shape == (64, 16) and bool((d.abs() == 1.0).all())
    assert torch.equal(d, dec.decode(net.eval(), False, y))
