"""CPU: the yardstick of the conv training kernels (tests/conv_train_helper.py) against the reference's own numbers,
and the conditions tests/test_conv_train_gpu.py's bars rest on.

  * the float64 restatement reproduces the gradients the reference's convNet recorded in float64
    (tests/golden/gen_conv_train.py), without and with a dropout multiplier, to float64 rounding;
  * E_ref (torch's fp32 autograd against float64) is positive and finite for every tensor and block of every GPU case,
    and no block's float64 norm is zero, so the per-block bar never skips and never divides by zero.  One block is
    exempt by construction: at B = 1 the LayerNorm bias's gradient is grad_out's only row itself, exact in any
    arithmetic, so its E_ref is 0 and its bar is equality;
  * every mutation misses the gradient bar tenfold on at least one case where it applies.
"""
import functools

import numpy as np
import pytest

import conv_train_helper as H

EXACT = {(1, "layer_norm.bias")}  # (B, block): the gradient is a copy of an input


@functools.lru_cache(maxsize=None)
def case_data(i):
    c = H.CASES[i]
    sd = H.case_weights(c)
    y, drop, gout = H.case_inputs(c)
    lg64, cx = H.forward64(sd, y, drop)
    g64 = H.backward64(cx, gout)
    lg32, g32 = H.torch_train(sd, y, drop, gout)
    return c, cx, gout, lg64, g64, lg32, H.block_errs(g32, g64)


def test_restatement_matches_reference_float64():
    fx = H.load_fixture()
    for mode in ("plain", "drop"):
        f = fx[mode]
        assert (f["drop"] is not None) == (mode == "drop")
        lg, g = H.train64(f["sd"], f["y"], f["drop"], f["gout"])
        assert np.abs(lg - f["logits64"]).max() < 1e-12
        got = H.fix_view(g)
        assert sorted(got) == sorted(f["g64"])
        for k, v in f["g64"].items():
            assert H.rel_err(got[k], v) < 1e-12, (mode, k)


def test_restatement_matches_torch_float64_autograd():
    import torch
    c = H.CASES[2]  # dropout multiplier, residuals, B past one FC tile
    sd, (y, drop, gout) = H.case_weights(c), H.case_inputs(c)
    lg, g = H.train64(sd, y, drop, gout)
    tl, tg = H.torch_train(sd, y, drop, gout, dtype=torch.float64)
    assert np.abs(lg - tl).max() < 1e-12
    assert max(H.block_errs(g, tg).values()) < 1e-11


def test_reference_fp32_is_within_its_own_error_scale():
    """The recorded fp32 gradients of the reference sit at fp32 rounding from its float64 ones: the scale E_ref has."""
    fx = H.load_fixture()
    for mode in ("plain", "drop"):
        f = fx[mode]
        for k, v in f["g64"].items():
            e = H.rel_err(f["g32"][k], v)
            assert 0.0 < e < 1e-5, (mode, k, e)


@pytest.mark.parametrize("i", range(len(H.CASES)), ids=[H.case_id(c) for c in H.CASES])
def test_e_ref_positive_and_no_zero_block(i):
    c, _, _, lg64, g64, lg32, eref = case_data(i)
    assert sorted(g64) == sorted(H.param_names(c.bias))
    assert np.abs(lg32 - lg64).max() < 1e-5
    for k, e in eref.items():  # block_errs has asserted every block's float64 norm positive
        if (c.B, k) in EXACT:
            assert e == 0.0, (k, e)
        else:
            assert np.isfinite(e) and 0.0 < e < 1e-4, (k, e)


@pytest.mark.parametrize("name", [m[0] for m in H.MUTATIONS])
def test_mutation_misses_the_bar_tenfold(name):
    applies = dict(H.MUTATIONS)[name]
    best = 0.0
    for i in (0, 1, 2, 5, 6, 3, 4):  # cheapest first
        c, cx, gout, _, g64, _, eref = case_data(i)
        if not applies(c):
            continue
        errs = H.block_errs(H.backward64(cx, gout, mutation=name), g64)
        best = max(best, max(errs[k] / (H.GRAD_FACTOR * eref[k]) for k in errs if eref[k] > 0.0))
        if best >= 10.0:
            return
    assert best >= 10.0, (name, best)


def test_c_abi_refuses_bad_arguments_before_any_gpu_call():
    import ctypes

    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    plan = ctypes.c_void_p()
    for N, E in ((100, 16), (32, 16), (2048, 16), (64, 8), (64, 24), (64, 528)):
        assert L.npd_conv_train_create(N, E, ctypes.byref(plan)) == -1 and not plan.value, (N, E)
    assert L.npd_conv_train_create(64, 512, ctypes.byref(plan)) == -2 and b"448" in L.npd_last_error()
    assert L.npd_conv_train_create(64, 16, None) == -1
    assert L.npd_conv_train_destroy(None) == -1
    sv, sc = ctypes.c_int64(), ctypes.c_int64()
    assert L.npd_conv_train_workspace(None, 4, ctypes.byref(sv), ctypes.byref(sc)) == -1
    assert L.npd_conv_train_forward(None, None, None, None, None, None, 4, None) == -1
    assert L.npd_conv_train_backward(None, None, None, None, None, None, None, None, 4, None) == -1


def test_train_conv_information_sets_flags_and_encoder():
    from neural_polar_decoder_amd import train_conv
    from neural_polar_decoder_amd.codes import polar_rs
    rs = polar_rs(64)
    n2c = [train_conv.stage_info(64, 22, k) for k in range(1, 23)]
    assert all(set(a) < set(b) for a, b in zip(n2c, n2c[1:])) and list(n2c[0]) == [rs[21]]
    assert np.array_equal(n2c[-1], np.sort(rs[:22]))
    assert np.array_equal(train_conv.stage_info(64, 22, 5, "c2n"), np.sort(rs[:5]))
    args = train_conv.parse_args(["--N", "64", "--K", "1", "--target_K", "22", "--embed_dim", "16"])
    assert (args.clip, args.dropout, args.model, args.max_len) == (0.25, 0.1, "conv", 64)
    import torch
    u = torch.ones(2, 8)
    u[:, 7] = -1
    assert torch.equal(train_conv.plotkin(u), -torch.ones(2, 8))  # the last row of F^{(x)3} is all ones
