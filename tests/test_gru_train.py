"""CRISP GRU training, CPU side: the float64 restatement (tests/train_helper.py) against fixtures recorded from the
reference (tests/golden/gen_train.py), the gradient bar and its mutations, and RNN_decoder.train_reason.

Bars.  The restatement matches each fixture's decoded and gradients to 1e-10 relative per tensor (2-norm): double
agreement, >= 1e5 x double epsilon for sums of <= 1e4 terms and three orders below any fp32-sized discrepancy.  E_ref of
a case is the error of torch's own fp32 autograd on the same inputs against the restatement (the largest per-tensor
relative error), computed here; the gradient bar is 16 E_ref: room for another summation order over the B N rows and
the 1 - 2 ulp of the gates' transcendentals, three orders under a dropped term.  Every mutation must miss that bar by
>= 10 x on every case it applies to.
"""
import numpy as np
import pytest

import train_helper as T

MODES = ("teacher", "student")


@pytest.fixture(scope="module", params=T.FIXTURES)
def fixture(request):
    fx = T.load_fixture(request.param)
    fx["name"] = request.param
    return fx


def _step(a, rev):
    return np.ascontiguousarray(a[:, ::-1]) if rev else a


def _run(fx, mode, mutation=None):
    """The restatement on a fixture's inputs: (decoded, grads) in the position frame, and the step-frame pieces."""
    rev, student = bool(fx["rev"]), mode == "student"
    gout_step = _step(fx[mode + ".gout"], rev)
    dec, bits, g = T.train64(fx["sd"], fx["y"], _step(fx["gt"], rev), int(fx["layers"]), bool(fx["onehot"]), fx["info"],
                             student, rev, gout_step, mutation=mutation)
    return _step(dec, rev), g, bits, gout_step


@pytest.mark.parametrize("mode", MODES)
def test_restatement_matches_the_reference(fixture, mode):
    dec, g, _, _ = _run(fixture, mode)
    e = T.rel_err(dec, fixture[mode + ".decoded"])
    print(f"{fixture['name']} {mode}: decoded {e:.2e}")
    assert e <= 1e-10
    assert sorted(g) == sorted(fixture[mode + ".g"])
    for k, ref in fixture[mode + ".g"].items():
        assert np.linalg.norm(ref.ravel()) > 0.0, k
        e = T.rel_err(g[k], ref)
        print(f"  {k}: {e:.2e}")
        assert e <= 1e-10, k


def test_student_forcing_leaves_unwritten_steps_at_one(fixture):
    """The reference tests ii, not jj, under reverse_order (rnn_all.py:493): the constant 1.0 sits at the steps outside
    info_inds in the step frame."""
    rev, N = bool(fixture["rev"]), int(fixture["N"])
    dec = _step(fixture["student.decoded"], rev)
    w = T.writes_of(N, fixture["info"], True)
    assert np.all(dec[:, ~w] == 1.0) and np.all(dec[:, w] != 1.0)
    assert np.all(_step(fixture["teacher.decoded"], rev) != 1.0)


@pytest.mark.parametrize("mode", MODES)
def test_gradient_bar_and_mutations(fixture, mode):
    fx = fixture
    rev, student = bool(fx["rev"]), mode == "student"
    N, F, layers, onehot = int(fx["N"]), int(fx["F"]), int(fx["layers"]), bool(fx["onehot"])
    _, g64, bits, gout_step = _run(fx, mode)
    eref = T.e_ref(fx["sd"], F, layers, N, onehot, fx["y"], bits, T.writes_of(N, fx["info"], student), gout_step, g64)
    bar = T.GRAD_FACTOR * eref
    print(f"{fx['name']} {mode}: E_ref {eref:.2e}, bar {bar:.2e}")
    assert 1e-8 < eref < 1e-6, "torch's fp32 autograd error left the range the bar was reasoned for"
    assert T.grad_err(g64, fx[mode + ".g"]) <= 1e-10
    for name, applies in T.MUTATIONS:
        if not applies(student, rev):
            continue
        dec_m, g_m, _, _ = _run(fx, mode, mutation=name)
        miss = max(T.grad_err(g_m, fx[mode + ".g"]), T.rel_err(dec_m, fx[mode + ".decoded"]))
        print(f"  mutation {name}: {miss:.2e} = {miss / bar:.1e} x bar")
        assert miss >= 10.0 * bar, name


def _decoder(decoding_type="y_input", onehot=False, precision="fp32", N=16):
    from neural_polar_decoder_amd.rnn import RNN_decoder
    return RNN_decoder(decoding_type, N, list(range(N // 2, N)), onehot=onehot, precision=precision)


def _net(cell="GRU", F=32, layers=1, N=16, onehot=False, y_hidden=0, y_depth=0, dropout=0.0, depth=1, bidir=False,
         ln=False, din=None):
    from neural_polar_decoder_amd.rnn import RNN_Model
    return RNN_Model(cell, N + 1 + int(onehot) if din is None else din, F, 1, layers, N, y_hidden, y_depth, "selu",
                     dropout, False, out_linear_depth=depth, bidirectional=bidir, use_layernorm=ln,
                     y_output_size=N if y_depth else None)


def test_train_reason_accepts_the_four_shapes():
    for F in (32, 64):
        for layers in (1, 2):
            for onehot in (False, True):
                dec = _decoder(onehot=onehot)
                assert dec.train_reason(_net(F=F, layers=layers, onehot=onehot)) is None
                assert dec.train_supported(_net(F=F, layers=layers, onehot=onehot)) is True


def test_train_reason_refuses_with_distinct_texts():
    refusals = {
        "lstm": _decoder().train_reason(_net(cell="LSTM")),
        "hidden128": _decoder().train_reason(_net(F=128)),
        "y_depth": _decoder().train_reason(_net(y_hidden=48, y_depth=2)),
        "y_h0": _decoder("y_h0").train_reason(_net(y_hidden=48, y_depth=2, din=1)),
        "layernorm": _decoder().train_reason(_net(ln=True)),
        "out_linear_depth": _decoder().train_reason(_net(depth=2, y_hidden=32)),
        "bidirectional": _decoder().train_reason(_net(bidir=True)),
        "dropout": _decoder().train_reason(_net(dropout=0.1)),
        "fp16x3": _decoder(precision="fp16x3").train_reason(_net()),
    }
    for k, v in refusals.items():
        assert isinstance(v, str) and v, k
    assert len(set(refusals.values())) == len(refusals), refusals
    assert "follow-up" in refusals["lstm"] and "follow-up" in refusals["hidden128"] and "follow-up" in refusals["fp16x3"]
    assert _decoder(N=12).train_reason(_net(N=12)) is not None          # N not a multiple of 8
    assert _decoder().train_reason(_net(din=20)) is not None            # input_size is not N + 1 + onehot


def test_refusals_raise_npd_error_before_any_gpu_call():
    import torch
    from neural_polar_decoder_amd import _lib
    y = torch.zeros(2, 16)
    with pytest.raises(_lib.NpdError, match="LSTM"):
        _decoder().decode(_net(cell="LSTM"), True, y, y, 1.0)
    with pytest.raises(_lib.NpdError, match="requires_grad"):
        _decoder().decode(_net(), True, y.clone().requires_grad_(), y, 1.0)
