"""GPU: every conv decoder layer and kernel variant of npd_conv*.hip against float64, per layer (the bar and the shape
table are tests/conv_layers_helper.py's), and the batch sizes, scales and calling conventions the other conv tests
leave out."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_layers_helper as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ("fp32", "fp16x3")
SMALL = [(48, 64), (64, 128)]


def words(E, N, B, seed):
    rng = np.random.default_rng(seed)
    return (np.where(rng.random((B, N)) < 0.5, -1.0, 1.0) + 0.8 * rng.standard_normal((B, N))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _kernel_row(E, N, prec):
    """The product kernels' 13 taps, logits and decisions on the row's compare words, run once per (row, precision)."""
    net = H.net_from(H.row_weights(E, N), E, N, precision=prec)
    return H.kernel_taps(net, torch.from_numpy(H.row_words(E, N)).to(DEV), H.compare_words(E, N))


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("E,N", H.ROWS)
def test_every_layer_against_float64(E, N, prec):
    """Every row of the shape table, both precisions: the ten conv layers' outputs, the FC1 and FC2 outputs and the logits
    within M x the fp32 restatement's own error against float64 (maximum and p99), the 1e-5 logit bar and the decisions,
    on word 0, the last word and words in between (the FC0 output: the next test).  The batch gives every persistent
    (weight-stationary) layer at least three items per block and a ragged last round, so the compared words include
    ones a block reaches only in its later rounds."""
    B, sel = H.batch_of(E, N), H.compare_words(E, N)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    for layer, kern, items, cols in H.persistent_layers(E, N, B, cu):
        assert items >= 3 * cols and items % cols != 0, (layer, kern, items, cols)
        assert sel[-2] * (items // B) >= 2 * cols  # besides the last word, one of a block's third or later round
    assert sel[0] == 0 and sel[-1] == B - 1
    taps, lg, dec = _kernel_row(E, N, prec)
    H.check_taps(taps, lg, dec, H.row_reference(E, N), label=f"({E},{N}) {prec}", names=H.BESIDES_FC0)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("E,N", H.ROWS)
def test_fc0_output_against_float64(E, N, prec):
    """The same bar on the FC0 output (tap 10, K = embed N terms per output), the first tap that left it: with one fp32
    accumulation chain over all of K the kernels stood at 8.7 - 14.5 x the restatement's error in fp32 from K = 12288
    up and at 11.3 x in fp16x3 at K = 65536 (a sequential fp32 sum on the CPU gave the same error), which the chains of
    1024 (fc_kernel) and 8160 terms (fc_split_wsp_kernel) brought to 1.6 - 2.7 x and 2.0 - 5.8 x (measured on an
    MI355X; tests/conv_layers_helper.py has every row)."""
    taps, lg, dec = _kernel_row(E, N, prec)
    H.check_taps(taps, lg, dec, H.row_reference(E, N), label=f"({E},{N}) {prec}", names=(H.FC0,))


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("E,N", SMALL)
def test_small_batches_equal_the_large_decode(E, N, prec):
    """B = 1 .. 257 (persistent grids clamped to the item count, FC row tiles that are mostly clamped rows, LayerNorm's
    ragged 4 rows per block): logits and decisions bit-identical to the first B rows of one decode of 257 words -- no
    per-word computation depends on the batch, and the activation scale of these inputs stays at its cap."""
    net = H.net_from(H.row_weights(E, N), E, N, precision=prec)
    y = torch.from_numpy(words(E, N, 257, 7 * E + N)).to(DEV)
    lg, dec = net.logits(y)
    for B in (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        lb, db = net.logits(y[:B].contiguous())
        assert torch.equal(lb, lg[:B]), (B, float((lb - lg[:B]).abs().max()))
        assert torch.equal(db, dec[:B]), B


@pytest.mark.parametrize("E,N", SMALL)
def test_mixed_scale_chunk(oracle, E, N):
    """fp16x3, one chunk of 64 words with word 7 multiplied by 3e4: the chunk shares one activation scale 2^SA, set by
    the large word, so the 63 ordinary words are split at SA ~ -2 instead of 4: an operand error of about 2^-23 relative,
    inside the fp32 rounding already there.  They stay within 1e-5 of float64 and word 7 within the 1e-4 of
    tests/test_conv_gpu.py's large-activation test (measured on an MI355X: 4.3e-7 and 3.7e-7 for the 63 words, 2.3e-6
    and 4.2e-6 for word 7)."""
    sd = H.row_weights(E, N)
    y = words(E, N, 64, 11 * E + N)
    y[7] *= 3e4
    lg, dec = H.net_from(sd, E, N, precision="fp16x3").logits(torch.from_numpy(y).to(DEV))
    lg, dec = lg.cpu().numpy(), dec.cpu().numpy()
    ref = oracle.conv_forward(y, sd, out_dtype=np.float64)
    err = np.abs(lg - ref).max(1)
    others = np.arange(64) != 7
    print((E, N), "63 words", err[others].max(), "word 7", err[7])
    assert np.isfinite(lg).all()
    assert err[others].max() < 1e-5, float(err[others].max())
    assert err[7] < 1e-4, float(err[7])
    sure = (np.abs(ref) > 1e-5) & others[:, None]
    assert np.array_equal(dec[sure], np.sign(ref)[sure])


def _degenerate_case(oracle, sd, E, N, prec, bias=True):
    y = H.row_words(E, N, 300)
    y[5] = 0.0
    y[131] = 0.75
    sel = np.array([0, 4, 5, 6, 130, 131, 132, 255, 256, 299])
    ref = H.Reference(oracle, y[sel], sd)
    assert ref.skip_share() <= 1e-3
    net = H.net_from(sd, E, N, precision=prec, bias=bias)
    taps, lg, dec = H.kernel_taps(net, torch.from_numpy(y).to(DEV), sel)
    H.check_taps(taps, lg, dec, ref, label=f"({E},{N}) {prec}")
    return taps


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("E,N", SMALL)
def test_zero_and_constant_words(oracle, E, N, prec):
    """An all-zero word and a constant word inside an ordinary batch, held to the per-layer bar with their neighbours."""
    _degenerate_case(oracle, H.row_weights(E, N), E, N, prec)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("E,N", SMALL)
def test_zero_weight_layer(oracle, E, N, prec):
    """Conv layer 4 with all-zero weights and bias: the host's weight scale takes its sw = 0 path, the layer's output is
    exactly zero and the next layer sees max |a| = 0; every tap stays on the per-layer bar (tap 4 exactly zero)."""
    sd = dict(H.row_weights(E, N))
    sd["layers3.0.weight"] = np.zeros_like(sd["layers3.0.weight"])
    sd["layers3.0.bias"] = np.zeros_like(sd["layers3.0.bias"])
    taps = _degenerate_case(oracle, sd, E, N, prec)
    assert not taps[4].any()


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("E,N", SMALL)
def test_without_conv_bias(oracle, E, N, prec):
    """dont_use_bias=True (Conv1d layers without bias; the Linear layers keep theirs), per layer."""
    sd = {k: v for k, v in H.row_weights(E, N).items() if not (k.startswith("layers") and k.endswith(".bias")
                                                              and not k.startswith("layersFin"))}
    _degenerate_case(oracle, sd, E, N, prec, bias=False)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("E,N", SMALL)
def test_direct_c_api_call(E, N, prec):
    """npd_conv_forward called directly: a workspace pre-filled with 0xFF bytes (NaN as floats) whose pointer sits 4 bytes
    into a larger allocation gives logits bit-identical to the wrapper's; the logits-only and decisions-only calls
    equal the two-output call."""
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    net = H.net_from(H.row_weights(E, N), E, N, precision=prec)
    B = 300
    y = torch.from_numpy(words(E, N, B, 13 * E + N)).to(DEV)
    lg0, dec0 = net.logits(y)
    h = net._get_handle(y.device)
    wsb = int(L.npd_conv_workspace_bytes(h, B))
    assert wsb > 0
    stream = _lib.stream_of(y.device)

    def call(want_lg, want_dec):
        ws = torch.full((wsb + 256,), 0xFF, dtype=torch.uint8, device=DEV)
        lg = torch.full((B, N), float("nan"), device=DEV) if want_lg else None
        dec = torch.full((B, N), float("nan"), device=DEV) if want_dec else None
        _lib.check(L.npd_conv_forward(h, _lib.ptr(y), _lib.ptr(lg), _lib.ptr(dec), ctypes.c_void_p(ws.data_ptr() + 4), B,
                                      stream), "npd_conv_forward")
        torch.cuda.synchronize()
        return lg, dec

    lg, dec = call(True, True)
    assert torch.equal(lg, lg0) and torch.equal(dec, dec0)
    lg1, none = call(True, False)
    assert none is None and torch.equal(lg1, lg0)
    none, dec1 = call(False, True)
    assert none is None and torch.equal(dec1, dec0)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    for tap in (-1, 13):  # refused before any launch
        rc = L.npd_conv_forward_tap(h, _lib.ptr(y), _lib.ptr(lg), None, tap, _lib.ptr(dec), _lib.ptr(ws), B, stream)
        assert rc == -1 and b"tap must be 0 .. 12" in L.npd_last_error()
