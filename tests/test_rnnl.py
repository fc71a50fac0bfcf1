"""CPU: GRU list decoding (RNN_decoder.list_decode, npd_gru_list_decode) -- what the fixtures mean and what is refused.

  * tests/rnnl_helper.py's float64 numpy restatement of the reference's list_decode reproduces, exactly, every fixture
    word the reference itself decodes alike in fp32 and float64 (``stable``): messages and the final list in list
    order.  This pins the fixtures' semantics without the reference.
  * list_decode / list_supported refuse the configurations the list kernel does not cover, before any GPU work.
  * the C entry points reject NULL handles and bad arguments; the CLI parses --rnn_list_size.
"""
import ctypes

import numpy as np
import pytest

import rnnl_helper as H


@pytest.mark.parametrize("name", list(H.FIXTURES))
def test_numpy_restatement_reproduces_the_stable_fixture_words(name):
    d, sd = H.load_fixture(name)
    N, K = int(d["N"]), int(d["K"])
    assert tuple(int(x) for x in d["Ls"]) == H.FIXTURES[name][1]
    for L in H.FIXTURES[name][1]:
        stable = d[f"stable_L{L}"]
        assert stable.mean() >= 0.99
        assert H.robust_mask(d, L).mean() >= 0.70
        r = H.list_decode_np(sd, N, d["info"], int(d["onehot"]), int(d["layers"]), d["y"], L,
                             pac_g=int(d["g"]) if int(d["pac"]) else 0)
        assert np.array_equal(r["msg"][stable], H.unpack_pm1(d[f"msg_L{L}"], K)[stable]), L
        assert np.array_equal(r["cand_msg"][stable], H.unpack_pm1(d[f"cand_L{L}"], K)[stable]), L
        err = np.abs(r["cand_metric"][stable] - d[f"cand_metric_L{L}"][stable]).max()
        assert err <= K * H.LOGIT_ATOL, (L, err)


def _net(rnn_type="GRU", F=32, layers=2, N=16, onehot=True, **kw):
    from neural_polar_decoder_amd.rnn import RNN_Model
    return RNN_Model(rnn_type, N + 1 + int(onehot), F, 1, layers, N, kw.pop("y_hidden", 0), 0, **kw).eval()


def test_list_decode_refuses_what_the_kernel_does_not_cover_without_a_gpu():
    import torch
    from neural_polar_decoder_amd import _lib, reference_polar_code
    from neural_polar_decoder_amd.rnn import RNN_decoder
    N, K = 16, 8
    code = reference_polar_code(N, K)
    info = np.asarray(code.info_positions)
    y = torch.zeros(4, N)
    ok = RNN_decoder("y_input", N, info, onehot=True)
    assert ok.list_supported(_net(), 1) and ok.list_supported(_net(F=64, layers=1), 8) and ok.list_supported(_net(), 5)
    cases = [
        (RNN_decoder("y_h0", N, info, onehot=True), _net(), 4, "y_input"),
        (RNN_decoder("y_input", N, info, onehot=True, reverse_order=True), _net(), 4, "reverse_order"),
        (RNN_decoder("y_input", N, info, onehot=True, precision="fp16x3"), _net(), 4, "fp32"),
        (RNN_decoder("y_input", N, info, onehot=True, precision="bf16"), _net(), 4, "fp32"),
        (ok, _net(bidirectional=True), 4, "unidirectional"),
        (ok, _net("LSTM"), 4, "LSTM"),
        (ok, _net(use_layernorm=True), 4, "LayerNorm"),
        (ok, _net(out_linear_depth=2, y_hidden=32), 4, "out_linear_depth"),
        (ok, _net(F=128), 4, "feature_size"),
        (ok, _net(F=16), 4, "feature_size"),
        (ok, _net(), 0, "list size"),
        (ok, _net(), 9, "list size"),
        (ok, _net(), 2.5, "list size"),
    ]
    for dec, net, L, word in cases:
        assert not dec.list_supported(net, L), word
        with pytest.raises(_lib.NpdError, match=word):
            dec.list_decode(net, y, code, L)


def test_c_entry_points_reject_null_and_bad_arguments():
    from neural_polar_decoder_amd import _lib
    from neural_polar_decoder_amd.polar import _CodeHandle
    L = _lib.load()
    one = ctypes.c_void_p(16)  # non-NULL, never dereferenced: every call below fails a check first
    code = _CodeHandle(16, np.arange(8, 16), 0)
    # a zeroed handle image: readable, and no configuration the list kernel covers (F = 0)
    buf = ctypes.create_string_buffer(4096)
    fake = ctypes.cast(buf, ctypes.c_void_p)
    assert L.npd_gru_list_supported(None, code.h, 4) < 0
    assert L.npd_gru_list_supported(fake, None, 4) < 0
    assert L.npd_gru_list_supported(fake, code.h, 4) == 0
    assert L.npd_gru_list_decode(None, code.h, one, None, 4, one, None, None, None, 4, None) == -1
    assert L.npd_gru_list_decode(fake, None, one, None, 4, one, None, None, None, 4, None) == -1
    assert L.npd_gru_list_decode(fake, code.h, one, None, 4, one, None, None, None, -1, None) == -1
    for bad in (0, 9, -3):
        assert L.npd_gru_list_decode(fake, code.h, one, None, bad, one, None, None, None, 4, None) == -1
        assert b"list_size" in L.npd_last_error()
    # the code's N (16) differs from the handle's (0)
    assert L.npd_gru_list_decode(fake, code.h, one, None, 4, one, None, None, None, 4, None) == -1
    # same N, but not an fp32 F = 32 / 64 GRU handle
    ctypes.memmove(buf, ctypes.byref(ctypes.c_int(16)), 4)
    assert L.npd_gru_list_decode(fake, code.h, one, None, 4, one, None, None, None, 4, None) == -2
    assert b"fp32" in L.npd_last_error()


def test_cli_parses_rnn_list_size():
    from neural_polar_decoder_amd import montecarlo
    a = montecarlo._parse_args(["--crisp", "--rnn_list_size", "4", "--N", "32", "--K", "16"])
    assert a.rnn_list_size == 4 and a.crisp
    assert montecarlo._parse_args(["--crisp"]).rnn_list_size is None
    with pytest.raises(SystemExit):
        montecarlo._parse_args(["--rnn_list_size", "4"])        # needs --crisp
    with pytest.raises(SystemExit):
        montecarlo._parse_args(["--crisp", "--rnn_list_size", "9"])
    assert issubclass(montecarlo.GRUListMonteCarlo, montecarlo.DecoderMonteCarlo)
