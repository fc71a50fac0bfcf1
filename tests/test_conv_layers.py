"""CPU: the per-layer conv check (tests/conv_layers_helper.py) on a plain fp32 evaluation, the negative controls that
show why the bar sits at the layers, and npd_conv_create's argument checks."""
import ctypes

import numpy as np
import pytest

import conv_layers_helper as H

DEFECTS = ("act16", "w16", "drop")


@pytest.mark.parametrize("E,N", H.SMALL_ROWS)
def test_clean_restatement_passes(oracle, E, N):
    """The torch fp32 restatement against itself (every ratio exactly 1) and against the float64 oracle: all 13 taps and
    the logits pass check_taps, the logit bar and the sign check included; the taps have the kernel's shapes."""
    ref = H.row_reference(E, N)
    rows = H.check_taps(ref.taps32, ref.lg32, np.sign(ref.lg32), ref, label=f"({E},{N}) clean")
    assert H.worst_ratio(rows)[0] == 1.0
    n = len(H.compare_words(E, N))
    shapes = [(n, E if t >= 8 else E // 2, N) for t in range(10)] + [(n, 4 * N), (n, N), (n, N)]
    assert [t.shape for t in ref.taps64] == shapes and [t.shape for t in ref.taps32] == shapes
    lg = oracle.conv_forward(H.row_words(E, N)[H.compare_words(E, N)], H.row_weights(E, N))
    assert np.array_equal(lg, ref.lg64.astype(np.float32))  # want_taps leaves the default output unchanged


@pytest.mark.parametrize("E,N", H.ROWS)
def test_sign_check_skips_at_most_one_logit_in_1000(E, N):
    """On every row's compare words the sign check leaves out at most 1 logit in 1,000 as within 1e-5 of zero."""
    ref = H.row_reference(E, N)
    share = ref.skip_share()
    print((E, N), "skipped", int(round(share * ref.lg64.size)), "of", ref.lg64.size)
    assert share <= 1e-3, ((E, N), share)


@pytest.mark.parametrize("layer", [1, 4, 7, 9])
@pytest.mark.parametrize("kind", DEFECTS)
def test_emulated_defect_is_rejected_per_layer(kind, layer):
    """Each emulated defect (fp16-rounded activations, fp16-rounded weights, one dropped input position for one output
    channel) in conv layer 1, 4, 7 or 9 fails check_taps at M = 8 on every small row, first at that layer's own tap; in
    layers 4 and 7 the old logits-only 1e-5 bar accepts it -- the reason for the per-layer bar."""
    for E, N in H.SMALL_ROWS:
        ref = H.row_reference(E, N)
        y, sd = H.row_words(E, N)[H.compare_words(E, N)], H.row_weights(E, N)
        lg, taps = H.torch_forward(y, sd, defect=(kind, layer))
        rows = H.tap_ratios(taps, lg, ref)
        for t in range(layer):  # upstream of the defect nothing moved
            assert rows[t][1] == rows[t][2] and rows[t][3] == rows[t][4]
        name, km, rm, kp, rp = rows[layer]
        print((E, N), kind, layer, "tap ratio max", km / rm, "p99", kp / rp, "logit diff", np.abs(lg - ref.lg64).max())
        assert km > H.M * rm or kp > H.M * rp, ((E, N), kind, layer, km / rm, kp / rp)
        with pytest.raises(AssertionError):
            H.check_taps(taps, lg, np.sign(lg), ref)
        if layer in (4, 7):
            H.check_logits_only(lg, np.sign(lg), ref.lg64)


def _conv_weight_count(N, E):
    h = E // 2
    n = (h * 1 * 7 + h) + 7 * (h * h * 7 + h) + (E * h * 7 + E) + (E * E * 7 + E)
    return n + 4 * N * E * N + 4 * N + N * 4 * N + N + N * N + N + 2 * N


def test_conv_create_argument_errors():
    """Every refusal of npd_conv_create: status -1, its message and a NULL out-handle, all decided before the first HIP
    call (no GPU needed, nothing read from the weights)."""
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    buf = np.zeros(16, dtype=np.float32)
    w = buf.ctypes.data_as(ctypes.c_void_p)
    cases = [((N, 64, _conv_weight_count(N, 64), 0), b"N must be a multiple of 64") for N in (32, 96, 1088)]
    cases += [((64, E, _conv_weight_count(64, E), 0), b"embed must be a multiple of 16") for E in (8, 24, 528)]
    cases += [((64, 64, _conv_weight_count(64, 64), 1), b"precision must be"),
              ((64, 64, _conv_weight_count(64, 64) + 1, 0), b"weight count does not match"),
              ((64, 64, _conv_weight_count(64, 64) - 1, 3), b"weight count does not match")]
    for (N, E, n, prec), msg in cases:
        out = ctypes.c_void_p(0xdead)
        rc = L.npd_conv_create(N, E, w, n, prec, ctypes.byref(out))
        assert rc == -1 and msg in L.npd_last_error() and out.value is None, (N, E, n, prec, rc, L.npd_last_error())
    out = ctypes.c_void_p(0xdead)
    assert L.npd_conv_create(64, 64, None, _conv_weight_count(64, 64), 0, ctypes.byref(out)) == -1
    assert b"weights is NULL" in L.npd_last_error() and out.value is None
    assert L.npd_conv_create(64, 64, w, _conv_weight_count(64, 64), 0, None) == -1
    assert b"out is NULL" in L.npd_last_error()
