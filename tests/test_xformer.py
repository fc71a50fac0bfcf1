"""CPU: the encoder and decoder transformer models' fixtures, float64 restatements, torch forwards, refusals and C
entry points.

The fixtures (tests/golden/gen_xformer.py) come from the reference's XFormerEndToEndEncoder / XFormerEndToEndDecoder,
run with the attention masks over the keys of each word.  tests/xformer_helper.py restates both in float64; this file
checks the restatements against the reference's recorded fp32 results, that the fixtures can tell a right model from a
wrong one (robust words, negative controls), and everything of the new surface that needs no GPU.

tol = max(2e-5, 4 e_ref) per fixture: 2e-5 is the project's LOGIT_ATOL, e_ref the reference's own fp32 error on the
compared logits (stored in the fixture); the factor 4 allows a second fp32 evaluation its own rounding of that size in
another order.
"""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import xformer_helper as X

CONTROL_WORDS = 16  # words per negative control (each control is one more float64 pass)
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------- fixtures and restatements
@pytest.mark.parametrize("name", X.FIXTURES)
def test_state_dict_loads_strictly(name):
    d, sd = X.fixture(name)
    net = X.build_net(name)
    keys = [str(k) for k in d["keys"]]
    assert list(net.state_dict().keys()) == keys
    if X.model_of(name) == "decoder":
        unused = ["Decoder.emb_auto.weight", "Decoder.position_enc_auto.pos_table", "Decoder.position_enc_cross.pos_table",
                  "Decoder.layer_stack.0.enc_attn.scalar.alpha", "Decoder.layer_stack.0.pos_ffn.scalar.alpha"]
        drop = "Decoder.emb_auto.weight"
    else:
        unused = ["Encoder.position_enc.pos_table", "Encoder.layer_stack.0.slf_attn.scalar.alpha",
                  "Encoder.layer_stack.0.pos_ffn.scalar.alpha"]
        drop = "Encoder.layer_stack.0.slf_attn.scalar.alpha"
    for k in unused:
        assert k in keys
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if k != drop}, strict=True)
    assert net.fused_supported() and net.fused_reason() == ""


def test_sinusoid_buffers_match_the_fixture():
    d, sd = X.fixture(X.DEC_FIXTURES[0])
    net = X.net_class("decoder")(X.xf_config("decoder", 16, 1))
    for k in ("position_enc_auto", "position_enc_cross"):
        assert np.array_equal(getattr(net.Decoder, k).pos_table.numpy(), sd[f"Decoder.{k}.pos_table"])
    assert not np.array_equal(sd["Decoder.position_enc_auto.pos_table"], sd["Decoder.position_enc_cross.pos_table"])


@pytest.mark.parametrize("name", X.DEC_FIXTURES)
def test_decoder_float64_restatement_reproduces_the_fixture(name):
    d, _ = X.fixture(name)
    info = d["info"]
    tol, e_ref = X.tol_of(d), float(d["e_ref"])
    f64 = X.forced64(name)
    err_forced = np.abs(f64 - d["forced_logits"].astype(np.float64))[:, info].max()
    bits, lg = X.free64(name)
    robust = X.robust_words(name)
    same = bits[:, info] == d["ref_bits"][:, info]
    agree = np.concatenate([np.ones((len(same), 1), bool), np.cumprod(same, 1)[:, :-1].astype(bool)], 1)
    err_free = np.abs(lg - d["ref_logits"].astype(np.float64))[:, info][agree].max()
    print(f"{name}: e_ref {e_ref:.3g} tol {tol:.3g} forced err {err_forced:.3g} free err {err_free:.3g}, "
          f"{int(robust.sum())} robust words of {len(robust)}")
    assert err_forced <= e_ref * (1 + 1e-9)
    assert robust.mean() >= 0.9
    assert np.array_equal(bits[robust], d["ref_bits"][robust].astype(np.float64))
    assert err_free <= tol
    frozen = np.setdiff1d(np.arange(int(d["N"])), info)
    assert np.all(d["ref_bits"][:, frozen] == 1) and np.all(d["ref_logits"][:, frozen] == 0)


@pytest.mark.parametrize("name", X.ENC_FIXTURES)
def test_encoder_float64_restatement_reproduces_the_fixture(name):
    d, _ = X.fixture(name)
    e_ref = float(d["e_ref"])
    bits, lg = X.free64(name)
    err = np.abs(lg - d["ref_logits"].astype(np.float64)).max()
    robust = X.robust_words(name)
    print(f"{name}: e_ref {e_ref:.3g} tol {X.tol_of(d):.3g} err {err:.3g}, {int(robust.sum())} robust words of {len(robust)}")
    assert err <= e_ref * (1 + 1e-9)
    assert robust.mean() >= 0.9
    assert np.array_equal(bits[robust], d["ref_bits"][robust].astype(np.float64))
    assert np.array_equal(d["ref_bits"], np.sign(d["ref_logits"]))  # the sign at every position, frozen ones included


@pytest.mark.parametrize("name", X.FIXTURES)
def test_fixture_logits_spread(name):
    """A model that ignored y (or the path) would give the same logit for every word."""
    d, _ = X.fixture(name)
    if X.model_of(name) == "decoder":
        spread = X.forced64(name)[:, d["info"]].std(0).min()
    else:
        spread = X.free64(name)[1].std(0).min()
    print(f"{name}: smallest per-position std {spread:.3g}, 100 tol = {100 * X.tol_of(d):.3g}")
    assert spread >= 100 * X.tol_of(d)


# ------------------------------------------------------------------------------------- the torch forwards
@pytest.mark.parametrize("name", X.FIXTURES)
def test_torch_forward_equals_the_references(name):
    """forward() (plain torch) against the reference's recorded forward() logits on 4 words; the decoder's expands
    each word to max_len rows, and its row b N + t at position t is the decode's logit at step t along that path."""
    d, _ = X.fixture(name)
    net = X.build_net(name)
    N, n = int(d["N"]), d["fwd_logits"].shape[0]
    tol = X.tol_of(d)
    with torch.no_grad():
        if X.model_of(name) == "decoder":
            n //= N
            y, forced = torch.from_numpy(d["y_forced"][:n]), torch.from_numpy(d["forced"][:n].astype(np.float32))
            out, bits, out_mask, logits = net(y, torch.ones(n, N).long(), forced, CPU)
            assert out.shape == (n * N, N, 2) and bits.shape == (n * N, N, 1) and logits.shape == (n * N, N, 1)
            assert out_mask.shape == (n * N, N)
            assert torch.equal(out_mask.reshape(n, N, N), torch.eye(N).expand(n, N, N))
            step = logits[:, :, 0].reshape(n, N, N).diagonal(dim1=1, dim2=2).numpy().astype(np.float64)
            err_step = np.abs(step - X.forced64(name)[:n])[:, d["info"]].max()
            print(f"{name}: forward's diagonal vs the float64 decode {err_step:.3g}")
            assert err_step <= tol
        else:
            y = torch.from_numpy(d["y"][:n])
            out, bits, out_mask, logits = net(y, torch.ones(n, N).long(), None, CPU)
            assert out.shape == (n, N, 2) and bits.shape == (n, N, 1) and logits.shape == (n, N, 1)
            assert out_mask.shape == (n, N)
    assert torch.equal(bits, logits.sign())
    assert torch.allclose(out[..., 1:], torch.sigmoid(logits)) and torch.allclose(out.sum(-1), torch.ones(out.shape[:-1]))
    err = np.abs(logits[:, :, 0].numpy().astype(np.float64) - d["fwd_logits"].astype(np.float64)).max()
    print(f"{name}: forward vs the reference's {err:.3g} (tol {tol:.3g})")
    assert err <= tol


# ------------------------------------------------------------------------------------- negative controls
def _moved_dec(name, **control):
    d, sd = X.fixture(name)
    n = CONTROL_WORDS
    _, lg = X.decode64_dec(sd, d["y_forced"][:n], d["is_info"], forced=d["forced"][:n], **control)
    return np.abs(lg - X.forced64(name)[:n])[:, d["info"]], d


@pytest.mark.parametrize("name", X.DEEP_DEC)
@pytest.mark.parametrize("control", ["causal", "cross_first_only", "rows_from_zero", "mem_table_10000"])
def test_decoder_negative_controls_move_the_logits(name, control):
    """What a wrong decoder would compute is far from the reference: a causal (KV-cached) self-attention,
    cross-attention in layer 0 only, emb_cross rows 0 .. N-1, and the num = 10000 table for the memory each move the
    float64 forced-path logits by more than 100 tol (median)."""
    diff, d = _moved_dec(name, **{control: True})
    moved = np.median(diff)
    print(f"{name} {control}: median move {moved:.3g}, 100 tol = {100 * X.tol_of(d):.3g}")
    assert moved > 100 * X.tol_of(d)


def test_one_layer_decoder_controls_that_change_nothing():
    """Why the >= 2-layer fixtures exist: with one layer, cross-attention 'in layer 0 only' is every layer (exactly 0),
    and token i's self-attention output reads only first-layer keys and values, which no mask changes."""
    name = X.DEC_FIXTURES[0]
    assert _moved_dec(name, cross_first_only=True)[0].max() == 0.0
    assert _moved_dec(name, causal=True)[0].max() < 1e-12


@pytest.mark.parametrize("name", X.DEEP_ENC)
def test_encoder_negative_control_moves_the_logits(name):
    """pos_emb rows 0 .. N-1 instead of 1 .. N (row 0 is the zero padding row)."""
    d, sd = X.fixture(name)
    n = CONTROL_WORDS
    moved = np.median(np.abs(X.forward64_enc(sd, d["y"][:n], rows_from_zero=True) - X.free64(name)[1][:n]))
    print(f"{name} rows_from_zero: median move {moved:.3g}, 100 tol = {100 * X.tol_of(d):.3g}")
    assert moved > 100 * X.tol_of(d)


# ------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("model", X.MODELS)
@pytest.mark.parametrize("kw,word", [(dict(embed_dim=128), "embed_dim"), (dict(n_head=4), "n_head"),
                                     (dict(N=128), "N 128"), (dict(N=8), "N 8"), (dict(n_layers=9), "n_layers"),
                                     (dict(N=32, max_len=64), "max_len")])
def test_unsupported_configurations_are_refused(model, kw, word):
    from neural_polar_decoder_amd import NpdError
    cfg = dict(N=32, n_layers=2, embed_dim=64, n_head=8)
    cfg.update(kw)
    net = X.net_class(model)(X.xf_config(model, **cfg)).eval()
    assert not net.fused_supported() and word in net.fused_reason() and model in net.fused_reason()
    N = cfg["N"]
    with pytest.raises(NpdError, match=word):
        net.decode(torch.zeros(2, N), [1, 2], torch.ones(2, N).long(), "cpu")
    with pytest.raises(NpdError, match=word):
        if model == "decoder":
            net.decode_logits(torch.zeros(2, N), [1, 2])
        else:
            net.logits(torch.zeros(2, N))


@pytest.mark.parametrize("model", X.MODELS)
def test_training_mode_mask_and_shapes_are_refused(model):
    from neural_polar_decoder_amd import NpdError
    net = X.net_class(model)(X.xf_config(model, 16, 1))
    net.train()
    with pytest.raises(NpdError, match="eval"):
        net.decode(torch.zeros(2, 16), [3, 5], torch.ones(2, 16).long(), "cpu")
    net.eval()
    mask = torch.ones(2, 16).long()
    mask[1, 7] = 0
    with pytest.raises(NpdError, match="all-ones mask"):
        net.decode(torch.zeros(2, 16), [3, 5], mask, "cpu")
    with pytest.raises(ValueError):
        net.decode(torch.zeros(2, 15), [3], torch.ones(2, 15).long(), "cpu")
    if model == "decoder":
        with pytest.raises(ValueError):
            net.decode_logits(torch.zeros(2, 16), [3, 16])
        with pytest.raises(ValueError):
            net.decode_logits(torch.zeros(2, 16), [3], forced=torch.ones(3, 16))


@pytest.mark.parametrize("model", X.MODELS)
def test_monte_carlo_refuses_an_unsupported_net(model):
    from neural_polar_decoder_amd import NpdError, reference_polar_code
    from neural_polar_decoder_amd.montecarlo import XFormerMonteCarlo
    net = X.net_class(model)(X.xf_config(model, 32, 2, n_head=4)).eval()
    with pytest.raises(NpdError, match="n_head"):
        XFormerMonteCarlo(reference_polar_code(32, 16), net, [1.0], 64, 64, device="cpu")


# ------------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("name", [X.DEC_FIXTURES[0], X.ENC_FIXTURES[1]])
def test_checkpoint_builds_the_model_it_names(name, tmp_path):
    from neural_polar_decoder_amd.datasets import xformer_from_checkpoint
    d, sd = X.fixture(name)
    model = X.model_of(name)
    args = X.xf_config(model, int(d["N"]), int(d["n_layers"]))
    args.K, args.code = int(d["K"]), "polar"
    path = str(tmp_path / "xf.pt")
    torch.save({"xformer": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "args": args, "step": 1}, path)
    net = xformer_from_checkpoint(path, device="cpu")
    assert type(net) is X.net_class(model) and not net.training and net.fused_supported()
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
    other = dict(sd)
    other.pop(next(iter(other)))
    with pytest.raises(RuntimeError):
        xformer_from_checkpoint({"xformer": {k: torch.from_numpy(v) for k, v in other.items()}, "args": args}, device="cpu")


def test_checkpoint_of_the_conv_model_is_still_refused():
    from neural_polar_decoder_amd.datasets import xformer_from_checkpoint
    with pytest.raises(NotImplementedError, match="conv"):
        xformer_from_checkpoint({"xformer": {}, "args": argparse.Namespace(model="conv")}, device="cpu")


# ------------------------------------------------------------------------------------- C entry points
def _count(model, N, L):
    return 192 * N + 641 + 66240 * L if model == "decoder" else 128 * N + 257 + 49728 * L


@pytest.mark.parametrize("model", X.MODELS)
def test_c_entry_points_reject_bad_arguments(model):
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    pre = "npd_xfdec" if model == "decoder" else "npd_xfenc"
    create = getattr(L, pre + "_create")
    out = ctypes.c_void_p()
    w = np.zeros(_count(model, 32, 2), np.float32)
    p = w.ctypes.data_as(ctypes.c_void_p)
    assert create(32, 64, 8, 2, p, w.size, None) == -1
    assert create(32, 64, 8, 2, None, w.size, ctypes.byref(out)) == -1 and b"weights" in L.npd_last_error()
    assert create(32, 128, 8, 2, p, w.size, ctypes.byref(out)) == -1 and b"embed_dim" in L.npd_last_error()
    assert create(32, 64, 4, 2, p, w.size, ctypes.byref(out)) == -1 and b"n_head" in L.npd_last_error()
    assert create(128, 64, 8, 2, p, w.size, ctypes.byref(out)) == -1 and b"N must" in L.npd_last_error()
    assert create(32, 64, 8, 0, p, w.size, ctypes.byref(out)) == -1 and b"n_layers" in L.npd_last_error()
    assert create(32, 64, 8, 9, p, w.size, ctypes.byref(out)) == -1
    assert create(32, 64, 8, 2, p, w.size - 1, ctypes.byref(out)) == -1 and b"count" in L.npd_last_error()
    assert create(32, 64, 8, 3, p, w.size, ctypes.byref(out)) == -1 and b"count" in L.npd_last_error()
    assert not out.value
    assert getattr(L, pre + "_destroy")(None) == -1 and b"handle" in L.npd_last_error()
    assert getattr(L, pre + "_workspace_bytes")(None, 4096) == -1 and b"handle" in L.npd_last_error()
    if model == "decoder":
        info = np.ones(32, np.uint8).ctypes.data_as(ctypes.c_void_p)
        assert L.npd_xfdec_decode(None, None, info, None, None, None, 4, None) == -1 and b"handle" in L.npd_last_error()
    else:
        assert L.npd_xfenc_forward(None, None, None, None, 4, None) == -1 and b"handle" in L.npd_last_error()


@pytest.mark.parametrize("name", [X.DEC_FIXTURES[0], X.ENC_FIXTURES[1]])
def test_packed_weights_follow_the_documented_order(name):
    d, sd = X.fixture(name)
    model, N, L = X.model_of(name), int(d["N"]), int(d["n_layers"])
    W = X.build_net(name)._packed()
    assert W.dtype == np.float32 and W.size == _count(model, N, L)
    E = 64
    if model == "decoder":
        assert np.array_equal(W[:(N + 1) * E], sd["Decoder.emb_cross.weight"].ravel())
        o = (N + 1) * E
        assert np.array_equal(W[o:o + N * E], sd["Decoder.position_enc_cross.pos_table"].ravel())
        o += N * E + 2 * E
        assert np.array_equal(W[o:o + 4 * E], sd["Decoder.emb_inputs.weight"].ravel())
        o += 4 * E
        assert np.array_equal(W[o:o + N * E], sd["Decoder.position_enc_auto.pos_table"].ravel())
        o += N * E + 2 * E
        assert np.array_equal(W[o:o + E * E], sd["Decoder.layer_stack.0.slf_attn.w_qs.weight"].ravel())
        o += 4 * E * E + 2 * E
        assert np.array_equal(W[o:o + E * E], sd["Decoder.layer_stack.0.enc_attn.w_qs.weight"].ravel())
    else:
        assert np.array_equal(W[:(N + 1) * E], sd["Encoder.pos_emb.weight"].ravel())
        o = (N + 1) * E + N * E + 2 * E
        assert np.array_equal(W[o:o + E * E], sd["Encoder.layer_stack.0.slf_attn.w_qs.weight"].ravel())
    assert np.array_equal(W[-65:-1], sd["Lin_Decoder.weight"].ravel()) and W[-1] == sd["Lin_Decoder.bias"][0]


# ------------------------------------------------------------------------------------- CLI
def test_cli_parses_the_xformer_flags():
    from neural_polar_decoder_amd.montecarlo import _parse_args
    a = _parse_args(["--N", "32", "--K", "16", "--xformer", "decoder", "--xformer_layers", "2",
                     "--xformer_checkpoint", "x.pt"])
    assert a.xformer == "decoder" and a.xformer_layers == 2 and a.xformer_checkpoint == "x.pt"
    b = _parse_args([])
    assert b.xformer is None and b.xformer_layers == 6 and b.xformer_checkpoint is None
    with pytest.raises(SystemExit):
        _parse_args(["--xformer", "gpt"])
