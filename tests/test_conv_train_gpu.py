"""convNet training on the fused kernels (npd_conv_train_forward / _backward), on the MI355X.

Every case of conv_train_helper.CASES runs convNet.train_logits and a backward with a given grad_out and is held to the
float64 restatement (tests/conv_train_helper.py):

  forward   |logit - float64 logit| <= conv_layers_helper.ATOL (1e-5, the project's conv logit bar)
  backward  every gradient tensor and every block (each tap of every conv weight, FC0's weight by position) within
            GRAD_FACTOR = 16 x E_ref of float64 (relative, 2-norm), E_ref = torch's fp32 autograd on the CPU on the same
            inputs, computed in the same run.  Where E_ref is 0 (the LayerNorm bias at B = 1, a copy of grad_out) the
            bar is equality.

The measured worst ratios error / E_ref per case are printed before they are asserted (DESIGN.md keeps the table).
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import conv_train_helper as H
from conv_layers_helper import ATOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = H.CASES[2]  # embed 32, B = 65, a dropout multiplier


def build(c, sd, dropout=0.0, precision="fp32", device=DEV):
    from neural_polar_decoder_amd.models import convNet
    cfg = types.SimpleNamespace(embed_dim=c.embed, max_len=c.N, N=c.N, dont_use_bias=not c.bias, dropout=dropout)
    net = convNet(cfg, precision=precision)
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return net.to(device).train()


def dev_t(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def run(net, y, drop, gout, stream=None):
    """One forward and backward: (logits, grads by name), numpy."""
    net.zero_grad()
    lg = net.train_logits(dev_t(y), dev_t(drop))
    assert lg.grad_fn is not None and lg.dtype == torch.float32 and lg.shape == y.shape and net.training
    (lg * dev_t(gout)).sum().backward()
    return lg.detach().cpu().numpy(), {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}


@functools.lru_cache(maxsize=None)
def reference(i):
    c = H.CASES[i]
    sd = H.case_weights(c)
    y, drop, gout = H.case_inputs(c)
    lg64, g64 = H.train64(sd, y, drop, gout)
    _, g32 = H.torch_train(sd, y, drop, gout)
    return sd, y, drop, gout, lg64, g64, H.block_errs(g32, g64)


@pytest.mark.parametrize("i", range(len(H.CASES)), ids=[H.case_id(c) for c in H.CASES])
def test_case_against_float64(i):
    c = H.CASES[i]
    sd, y, drop, gout, lg64, g64, eref = reference(i)
    net = build(c, sd)
    lg, g = run(net, y, drop, gout)
    assert sorted(g) == sorted(g64)
    err = H.block_errs(g, g64)
    elog = float(np.abs(lg - lg64).max())
    worst = max(((err[k] / eref[k], k) for k in err if eref[k] > 0.0))
    print(f"\n{H.case_id(c)}: logits {elog:.3g}; worst gradient error / E_ref {worst[0]:.2f} ({worst[1]}); "
          f"worst whole tensor {max(err[k] / eref[k] for k in g64 if eref[k] > 0.0):.2f}")
    assert elog <= ATOL
    for k in err:
        assert err[k] <= H.GRAD_FACTOR * eref[k], (k, err[k], eref[k])


def test_identical_calls_identical_bits():
    sd, y, drop, gout = reference(2)[:4]
    net = build(SMALL, sd)
    l1, g1 = run(net, y, drop, gout)
    l2, g2 = run(net, y, drop, gout)
    assert np.array_equal(l1, l2)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k


def test_next_forward_sees_stepped_weights():
    sd, y, drop, gout = reference(2)[:4]
    net = build(SMALL, sd)
    l0, _ = run(net, y, drop, gout)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(p.grad, alpha=-1e-2)
    lg = net.train_logits(dev_t(y), dev_t(drop)).detach().cpu().numpy()
    sd2 = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    lg64, _ = H.forward64(sd2, y, drop)
    assert np.abs(lg - lg64).max() <= ATOL
    assert np.abs(lg - l0).max() > 100 * ATOL


def test_two_forwards_then_one_backward_on_a_shared_plan():
    sd, y, drop, gout = reference(2)[:4]
    net = build(SMALL, sd)
    _, g_alone = run(net, y, drop, gout)
    net.zero_grad()
    l1 = net.train_logits(dev_t(y), dev_t(drop))
    l2 = net.train_logits(dev_t(y[::-1].copy()), None)  # rewrites the plan's images, own saved buffer
    (l1 * dev_t(gout)).sum().backward()
    for k, p in net.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy(), g_alone[k]), k
    assert l2.grad_fn is not None


def test_retain_graph():
    sd, y, drop, gout = reference(2)[:4]
    net = build(SMALL, sd)
    _, g1 = run(net, y, drop, gout)
    net.zero_grad()
    loss = (net.train_logits(dev_t(y), dev_t(drop)) * dev_t(gout)).sum()
    loss.backward(retain_graph=True)
    loss.backward()
    for k, p in net.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy(), g1[k] + g1[k]), k


def test_side_stream():
    sd, y, drop, gout = reference(2)[:4]
    net = build(SMALL, sd)
    l1, g1 = run(net, y, drop, gout)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        l2, g2 = run(net, y, drop, gout)
    torch.cuda.current_stream(DEV).wait_stream(s)
    assert np.array_equal(l1, l2)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k


def test_inplace_parameter_change_before_backward_raises():
    sd, y, drop, gout = reference(2)[:4]
    net = build(SMALL, sd)
    lg = net.train_logits(dev_t(y), dev_t(drop))
    with torch.no_grad():
        net.layers3[0].weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (lg * dev_t(gout)).sum().backward()


def test_eval_decode_after_a_training_step_equals_a_fresh_module():
    sd, y, drop, gout = reference(2)[:4]
    net = build(SMALL, sd, dropout=0.1)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    out = net(dev_t(y), torch.ones_like(dev_t(y)).long(), None, DEV)
    (out[3][:, :, 0] * dev_t(gout)).sum().backward()
    opt.step()
    net.eval()
    with torch.no_grad():
        lg, dec = net.logits(dev_t(y))
    fresh = build(SMALL, {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}).eval()
    with torch.no_grad():
        lf, df = fresh.logits(dev_t(y))
    assert torch.equal(lg, lf) and torch.equal(dec, df)


def test_forward_returns_the_reference_five_values():
    sd, y, drop, gout = reference(2)[:4]
    net = build(SMALL, sd)
    mask = torch.ones(y.shape, device=DEV).long()
    output, dec, out_mask, logits, in4 = net(dev_t(y), mask, None, DEV)
    B, N = y.shape
    assert output.shape == (B, N, 2) and dec.shape == (B, N, 1) and logits.shape == (B, N, 1) and out_mask is mask
    assert logits.grad_fn is not None and not in4.requires_grad and in4.shape == (B, SMALL.embed // 2, N)
    assert torch.equal(dec, logits.detach().sign())
    assert torch.allclose(output[:, :, 1], torch.sigmoid(logits[:, :, 0]))
    net.eval()
    with torch.no_grad():
        e = net(dev_t(y), mask, None, DEV)
    assert float((e[4] - in4).abs().max()) < 1e-5          # input4 does not pass the dropout layer
    assert float((e[3] - logits.detach()).abs().max()) < 1e-4       # dropout 0: the training logits are the eval logits


def test_dropout_is_drawn_from_torchs_generator():
    sd, y = reference(2)[0], reference(2)[1]
    net = build(SMALL, sd, dropout=0.5)
    torch.manual_seed(5)
    a = net.train_logits(dev_t(y)).detach()
    b = net.train_logits(dev_t(y)).detach()
    torch.manual_seed(5)
    c = net.train_logits(dev_t(y)).detach()
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_absent_biases_take_no_gradient():
    c = H.CASES[1]
    sd, y, drop, gout = reference(1)[:4]
    net = build(c, sd)
    _, g = run(net, y, drop, gout)
    assert all(m.bias is None for m in net._convs()) and "layers1.0.bias" not in g and "layersFin.0.bias" in g


def test_every_train_reason_refusal():
    from neural_polar_decoder_amd._lib import NpdError
    sd, y = reference(0)[0], reference(0)[1]
    c = H.CASES[0]
    net = build(c, sd)
    assert net.train_supported() and net.train_reason() is None
    split = build(c, sd, precision="fp16x3")
    assert "fp32" in split.train_reason() and not split.train_supported()
    host = build(c, sd, device="cpu")
    assert "on the GPU" in host.train_reason()
    yg = dev_t(y).requires_grad_()
    assert "requires_grad" in net.train_reason(yg)
    for n_, args in ((split, (dev_t(y),)), (host, (dev_t(y),)), (net, (yg,))):
        with pytest.raises(NpdError):
            n_.train_logits(*args)
    with pytest.raises(NpdError):
        host(torch.from_numpy(y), torch.ones(y.shape).long(), None, "cpu")


def test_c_abi_zero_batch_and_null_arguments():
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    plan = ctypes.c_void_p()
    with torch.cuda.device(DEV):
        assert L.npd_conv_train_create(64, 16, ctypes.byref(plan)) == 0
        sv, sc = ctypes.c_int64(), ctypes.c_int64()
        assert L.npd_conv_train_workspace(plan, 0, ctypes.byref(sv), ctypes.byref(sc)) == 0
        nw = sum(v.size for v in reference(0)[0].values())
        w = torch.zeros(nw, device=DEV)
        g = torch.full((nw,), 7.0, device=DEV)
        st = _lib.stream_of(torch.device(DEV))
        assert L.npd_conv_train_backward(plan, _lib.ptr(w), None, None, None, None, None, _lib.ptr(g), 0, st) == 0
        assert float(g.abs().max()) == 0.0
        assert L.npd_conv_train_forward(plan, _lib.ptr(w), None, None, None, None, 0, st) == 0
        assert L.npd_conv_train_forward(plan, _lib.ptr(w), None, None, None, None, 4, st) == -1
        assert L.npd_conv_train_forward(plan, None, None, None, None, None, 4, st) == -1
        assert L.npd_conv_train_backward(plan, _lib.ptr(w), None, None, None, None, None, None, 4, st) == -1
        assert L.npd_conv_train_destroy(plan) == 0


def test_train_conv_five_steps_and_checkpoint(tmp_path):
    from neural_polar_decoder_amd import train_conv
    from neural_polar_decoder_amd.datasets import convnet_from_checkpoint
    path = str(tmp_path / "stage.pt")
    args = train_conv.parse_args(["--N", "64", "--K", "3", "--target_K", "22", "--embed_dim", "16", "--batch_size", "64",
                                  "--num_steps", "5", "--dec_train_snr", "-4", "--save_path", path, "--print_freq", "0"])
    net, info, losses = train_conv.train(args, device=DEV, log=lambda *_: None)
    assert len(losses) == 5 and all(np.isfinite(losses)) and len(info) == 3
    ck = convnet_from_checkpoint(path, device=DEV)
    for k, v in net.state_dict().items():
        assert torch.equal(ck.state_dict()[k], v), k
    y = torch.randn(8, 64, device=DEV)
    dec, _ = ck.decode(y, info, None, DEV)
    assert dec.shape == (8, 64, 1)
    args2 = train_conv.parse_args(["--N", "64", "--K", "4", "--target_K", "22", "--embed_dim", "16", "--batch_size", "64",
                                   "--num_steps", "2", "--load_previous", "--load_path", path, "--print_freq", "0"])
    _, info2, losses2 = train_conv.train(args2, device=DEV, log=lambda *_: None)
    assert len(info2) == 4 and set(info) <= set(info2) and len(losses2) == 2
