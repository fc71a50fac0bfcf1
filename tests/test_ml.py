"""CPU: the ML / bitwise-MAP codebook convention (codes.generator_rows, codes.all_message_bits) against the oracle's
encoders, the fixtures' stored indices against a float64 argmax, and the new entry points' argument checks."""
import ctypes

import numpy as np
import pytest

from conftest import golden

FIXTURES = ["ml_polar_8_2", "ml_polar_16_8", "ml_polar_32_16", "ml_polar_64_12", "ml_pac_32_10", "ml_pac_16_5"]


@pytest.mark.parametrize("name", FIXTURES)
def test_generator_rows_span_the_oracle_codebook(name, oracle):
    from neural_polar_decoder_amd.codes import all_message_bits, codebook_masks, generator_rows, masks_to_pm1
    d = golden(name + ".npz")
    N, K, g, info = int(d["N"]), int(d["K"]), int(d["g"]), d["info"]
    amb = all_message_bits(K)
    assert amb.shape == (2 ** K, K) and np.all(amb[0] == 1.0)
    i = np.arange(2 ** K)
    for k in range(K):                                          # dec2bitarray, MSB first (utils.py:170-192)
        assert np.array_equal(amb[:, k], 1.0 - 2.0 * ((i >> (K - 1 - k)) & 1))
    x = oracle.pac_encode(amb, N, info, g=g) if int(d["pac"]) else oracle.encode_plotkin(amb, N, info)
    rows = generator_rows(N, info, g if int(d["pac"]) else 0)
    assert rows.dtype == np.uint64 and rows.shape == (K,)
    assert np.array_equal(masks_to_pm1(codebook_masks(rows), N, np.float32), x)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_indices_are_the_float64_argmax(name):
    from neural_polar_decoder_amd.codes import codebook_masks, generator_rows, masks_to_pm1
    d = golden(name + ".npz")
    N, g = int(d["N"]), int(d["g"])
    cb = masks_to_pm1(codebook_masks(generator_rows(N, d["info"], g if int(d["pac"]) else 0)), N)
    corr = d["y"].astype(np.float64) @ cb.T
    assert np.array_equal(corr.argmax(1), d["idx"])
    top2 = np.partition(corr, -2, axis=1)[:, -2:]
    eps = 2.0 * N * 2.0 ** -24 * np.abs(d["y"].astype(np.float64)).sum(1)
    assert np.all(top2[:, 1] - top2[:, 0] >= 4 * eps)


def _handle(N, K, g=0):
    from neural_polar_decoder_amd.polar import _CodeHandle
    return _CodeHandle(N, np.arange(N - K, N), g)


def test_unsupported_shapes_and_missing_outputs_are_rejected_without_a_gpu():
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    one = ctypes.c_void_p(16)      # a non-NULL pointer that is never dereferenced: every call fails its checks first
    for N, K, is_map in [(128, 16, 0), (64, 23, 0), (64, 17, 1), (128, 8, 1), (4, 2, 0)]:
        h = _handle(N, K)
        assert L.npd_ml_supported(h.h, is_map) == 0
        if is_map:
            assert L.npd_map_decode(h.h, one, 1.0, one, one, 4, None) == -2
        else:
            assert L.npd_ml_decode(h.h, one, one, one, one, 4, None) == -2
        assert L.npd_last_error()
    for N, K, g in [(64, 22, 0), (32, 16, 0), (8, 1, 0), (32, 10, 53)]:
        h = _handle(N, K, g)
        assert L.npd_ml_supported(h.h, 0) == 1
        assert L.npd_ml_supported(h.h, 1) == (1 if K <= 16 else 0)
    h = _handle(32, 16)
    assert L.npd_ml_decode(h.h, one, None, None, None, 4, None) < 0          # no output requested
    assert b"output" in L.npd_last_error()
    assert L.npd_map_decode(h.h, one, 1.0, None, None, 4, None) < 0
    assert L.npd_ml_decode(h.h, None, one, None, None, 4, None) < 0          # y is NULL
    assert L.npd_map_decode(h.h, one, -1.0, one, None, 4, None) < 0          # negative scale
    assert L.npd_ml_supported(None, 0) < 0
    assert L.npd_ml_decode(h.h, None, one, None, None, 0, None) == 0         # B == 0: a no-op
    assert L.npd_map_decode(h.h, None, 1.0, one, None, 0, None) == 0


def test_python_surface_exists_and_reports_support():
    import neural_polar_decoder_amd as npd
    from neural_polar_decoder_amd import montecarlo
    assert npd.reference_polar_code(32, 16).ml_supported() and npd.reference_polar_code(32, 16).ml_supported(map=True)
    assert npd.reference_polar_code(64, 22).ml_supported() and not npd.reference_polar_code(64, 22).ml_supported(map=True)
    assert not npd.reference_polar_code(128, 16).ml_supported()
    assert npd.PAC(None, 32, 10, 53).ml_supported(map=True)
    for name in ("ml_decode", "bitwise_MAP"):
        assert callable(getattr(npd.PolarCode, name)) and callable(getattr(npd.PAC, name))
    assert issubclass(montecarlo.MLMonteCarlo, montecarlo.MonteCarlo)
    assert issubclass(montecarlo.MAPMonteCarlo, montecarlo.MonteCarlo)
