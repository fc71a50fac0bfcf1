"""CPU: the C-ABI library loads, exports exactly what include/npd.h declares, and validates
arguments without touching a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "npd.h")
LIB = os.path.join(ROOT, "neural_polar_decoder_amd", "libnpd.so")


def declared_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(npd_[a-z0-9_]+)\s*\(", src)))


def test_library_exists():
    assert os.path.exists(LIB), "build libnpd.so first (make lib / __graft_entry__.build())"


def test_exports_every_declared_symbol():
    syms = declared_symbols()
    assert len(syms) >= 18
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (npd_[a-z0-9_]+)", out))
    missing = [s for s in syms if s not in exported]
    assert not missing, missing
    L = ctypes.CDLL(LIB)
    for s in syms:
        assert getattr(L, s) is not None


def test_python_binding_matches_header():
    from neural_polar_decoder_amd import _lib
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert bound == set(declared_symbols())


def test_abi_and_device_count_without_gpu():
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    assert L.npd_abi_version() == 1
    assert L.npd_device_count() >= 0


def test_code_create_argument_errors():
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    out = ctypes.c_void_p()
    info = np.arange(4, dtype=np.int32)
    p = info.ctypes.data_as(ctypes.c_void_p)
    assert L.npd_code_create(48, 4, p, 0, 1000.0, ctypes.byref(out)) == -1      # not a power of two
    assert b"power of two" in L.npd_last_error()
    assert L.npd_code_create(512, 4, p, 0, 1000.0, ctypes.byref(out)) == -1     # too long
    bad = np.array([3, 1], dtype=np.int32)
    assert L.npd_code_create(8, 2, bad.ctypes.data_as(ctypes.c_void_p), 0, 1000.0, ctypes.byref(out)) == -1
    assert L.npd_code_create(8, 4, p, 91, 1000.0, ctypes.byref(out)) == 0       # valid PAC handle (host only)
    assert out.value
    assert L.npd_code_destroy(out) == 0


def _rnn_weight_count(gates, N, F, layers, onehot):
    din = N + (2 if onehot else 1)
    n = gates * F * din + gates * F * F + 2 * gates * F
    if layers == 2:
        n += 2 * gates * F * F + 2 * gates * F
    return n + F + 1


def test_rnn_create_argument_errors():
    """Every refusal of npd_gru_create / npd_rnn_create / npd_rnn_create_ex: status -1, its message, a NULL out-handle.
    All of them are decided before the first HIP call, so nothing is allocated and no GPU is needed."""
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    # read only by the LayerNorm fold (n_weights floats, before npd_gru_create counts them): large enough for that case
    buf = np.zeros(8192, dtype=np.float32)
    w = buf.ctypes.data_as(ctypes.c_void_p)
    ln = np.ones(64, dtype=np.float32)
    lnp = ln.ctypes.data_as(ctypes.c_void_p)

    def nw(N, F, layers, onehot=1, gates=3):
        return _rnn_weight_count(gates, N, F, layers, onehot)

    # (N, F, layers, onehot, n_weights, precision), message
    gru_cases = [
        ((12, 32, 1, 1, nw(12, 32, 1), 0), b"multiple of 8"),
        ((16, 48, 1, 1, nw(16, 48, 1), 0), b"hidden size F must be"),
        ((16, 128, 1, 1, nw(16, 128, 1), 3), b"cover F <= 64"),
        ((256, 512, 2, 1, nw(256, 512, 2), 0), b"needs N <= 248"),
        ((16, 32, 3, 1, nw(16, 32, 2), 0), b"1 or 2 GRU layers"),
        ((16, 32, 1, 1, nw(16, 32, 1), 4), b"precision must be"),
        ((8, 32, 1, 1, nw(8, 32, 1), 3), b"N % 16"),
        ((16, 32, 1, 1, nw(16, 32, 1) + 1, 0), b"weight count does not match (N, F"),
        ((16, 32, 1, 1, nw(16, 32, 1) - 1, 0), b"weight count does not match (N, F"),
        ((16, 64, 2, 0, nw(16, 64, 2, 1), 0), b"weight count does not match (N, F"),
    ]
    for (N, F, layers, onehot, n, prec), msg in gru_cases:
        out = ctypes.c_void_p(0xdead)
        rc = L.npd_gru_create(N, F, layers, onehot, w, n, prec, ctypes.byref(out))
        assert rc == -1 and msg in L.npd_last_error() and out.value is None, (N, F, layers, prec, rc, L.npd_last_error())
    out = ctypes.c_void_p(0xdead)
    assert L.npd_gru_create(16, 32, 1, 1, None, nw(16, 32, 1), 0, ctypes.byref(out)) == -1
    assert b"weights is NULL" in L.npd_last_error() and out.value is None
    assert L.npd_gru_create(16, 32, 1, 1, w, nw(16, 32, 1), 0, None) == -1
    assert b"out is NULL" in L.npd_last_error()

    # (cell, N, F, layers, onehot, n_weights, precision), message
    rnn_cases = [
        ((2, 16, 32, 1, 1, nw(16, 32, 1), 0), b"cell must be"),
        ((1, 16, 32, 1, 1, nw(16, 32, 1, gates=4), 3), b"LSTM cells run fp32"),
        ((1, 16, 32, 1, 1, nw(16, 32, 1, gates=4) + 1, 0), b"(LSTM"),
        ((1, 16, 64, 2, 1, nw(16, 64, 2, gates=4) - 1, 0), b"(LSTM"),
        ((1, 12, 32, 1, 1, nw(12, 32, 1, gates=4), 0), b"multiple of 8"),
        ((1, 16, 48, 1, 1, nw(16, 48, 1, gates=4), 0), b"LSTM hidden size F must be"),
        ((1, 256, 512, 2, 1, nw(256, 512, 2, gates=4), 0), b"needs N <= 248"),
        ((1, 16, 32, 3, 1, nw(16, 32, 2, gates=4), 0), b"1 or 2 layers"),
        ((0, 16, 48, 1, 1, nw(16, 48, 1), 0), b"npd_gru_create: hidden size F must be"),   # cell 0: the GRU ladder
    ]
    for (cell, N, F, layers, onehot, n, prec), msg in rnn_cases:
        out = ctypes.c_void_p(0xdead)
        rc = L.npd_rnn_create(cell, N, F, layers, onehot, w, n, prec, ctypes.byref(out))
        assert rc == -1 and msg in L.npd_last_error() and out.value is None, (cell, N, F, layers, prec, rc,
                                                                             L.npd_last_error())

    def head_n(F, depth, H):
        return H * F + H + (depth - 2) * (H * H + H) + H + 1

    # (cell, N, F, layers, n_weights, precision, ln_weight, ln_bias, head_depth, head_hidden, head_weights, n_head), message
    ex_cases = [
        ((0, 16, 32, 1, nw(16, 32, 1), 0, None, None, 9, 20, w, head_n(32, 9, 20)), b"head_depth must be 1 .. 8"),
        ((0, 16, 32, 1, nw(16, 32, 1), 0, None, None, 0, 20, w, 0), b"head_depth must be 1 .. 8"),
        ((0, 16, 32, 1, nw(16, 32, 1), 0, lnp, lnp, 2, 20, w, head_n(32, 2, 20)), b"not fused"),
        ((0, 16, 128, 1, nw(16, 128, 1), 0, None, None, 2, 20, w, head_n(128, 2, 20)),
         b"out_linear_depth > 1 head runs on the fp32 GRU kernel"),
        ((0, 16, 32, 1, nw(16, 32, 1), 0, None, None, 2, 129, w, head_n(32, 2, 129)),
         b"out_linear_depth > 1 head runs on the fp32 GRU kernel"),
        ((0, 16, 32, 1, nw(16, 32, 1), 0, None, None, 2, 20, None, head_n(32, 2, 20)), b"null pointer"),
        ((0, 16, 32, 1, nw(16, 32, 1) + 1, 0, None, None, 2, 20, w, head_n(32, 2, 20)),
         b"weight count does not match (N, F"),
        ((0, 16, 32, 1, nw(16, 32, 1), 3, lnp, lnp, 1, 0, None, 0), b"LayerNorm head runs on the fp32 GRU kernel"),
        ((1, 16, 32, 1, nw(16, 32, 1, gates=4), 0, lnp, lnp, 1, 0, None, 0),
         b"LayerNorm head runs on the fp32 GRU kernel"),
        ((0, 16, 32, 1, nw(16, 32, 1), 0, lnp, None, 1, 0, None, 0), b"null pointer"),
        ((0, 16, 32, 1, nw(16, 32, 1) + 1, 0, lnp, lnp, 1, 0, None, 0), b"weight count does not match (N, F"),
        ((2, 16, 32, 1, nw(16, 32, 1), 0, None, None, 1, 0, None, 0), b"cell must be"),    # plain head: npd_rnn_create's
    ]
    for (cell, N, F, layers, n, prec, lw, lb, depth, H, hw, nh), msg in ex_cases:
        out = ctypes.c_void_p(0xdead)
        rc = L.npd_rnn_create_ex(cell, N, F, layers, 1, w, n, prec, lw, lb, 1e-5, depth, H, hw, nh, ctypes.byref(out))
        assert rc == -1 and msg in L.npd_last_error() and out.value is None, (cell, F, prec, depth, H, rc,
                                                                             L.npd_last_error())


@pytest.mark.gpu
def test_rnn_create_at_the_lds_limit():
    """F = 512 with 2 layers keeps (2 F + N + 8) * 128 bytes in LDS: N = 248 is 163 840 bytes, all 160 KiB, and is
    accepted; N = 256 is refused with NPD_EINVAL before any HIP call; F = 512 with 1 layer takes N = 256.  Both cells,
    through npd_gru_create and npd_rnn_create.  (An accepted create uploads its images, hence the gpu mark; that the
    accepted edge also decodes correctly is tests/test_forced_path_gpu.py's N = 248 rows.)"""
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    assert (2 * 512 + 248 + 8) * 128 == 160 * 1024
    buf = np.zeros(_rnn_weight_count(4, 256, 512, 2, 1), dtype=np.float32)
    w = buf.ctypes.data_as(ctypes.c_void_p)
    for layers, N, ok in ((2, 248, True), (2, 256, False), (1, 256, True)):
        creates = [("npd_gru_create", lambda out: L.npd_gru_create(N, 512, layers, 1, w,
                                                                   _rnn_weight_count(3, N, 512, layers, 1), 0, out))]
        for cell, gates in ((0, 3), (1, 4)):
            creates.append((f"npd_rnn_create cell {cell}", lambda out, cell=cell, gates=gates: L.npd_rnn_create(
                cell, N, 512, layers, 1, w, _rnn_weight_count(gates, N, 512, layers, 1), 0, out)))
        for who, create in creates:
            out = ctypes.c_void_p(0xdead)
            rc = create(ctypes.byref(out))
            if ok:
                assert rc == 0 and out.value, (who, layers, N, rc, L.npd_last_error())
                assert L.npd_gru_destroy(out) == 0
            else:
                assert rc == -1 and out.value is None, (who, layers, N, rc)
                assert b"needs N <= 248" in L.npd_last_error() and b"160 KiB" in L.npd_last_error()


def test_null_pointer_errors_are_reported_not_fatal():
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    assert L.npd_sc_decode(None, None, 1.0, None, None, None, None, 16, None) == -1
    assert L.npd_awgn(None, None, 16, 6, 1.0, 0, 0, 0, None) == -1             # N % 4 != 0
    assert L.npd_count_errors(None, None, 4, 4, None, None) == -1
    assert L.npd_sc_decode_lse(None, None, 1.0, 1, None, None, 16, None) == -1
    assert L.npd_sc_decode_soft(None, None, 1.0, 1, None, None, None, 16, None) == -1
    assert L.npd_sc_decode_soft_new(None, None, 1.0, None, None, None, 16, None) == -1


def test_product_path_has_no_cpu_fallback():
    """Host inputs are staged to the GPU; with no GPU visible every compute call raises."""
    import torch
    from neural_polar_decoder_amd import NpdError, errors_bler, reference_polar_code
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: host tensors are staged to it")
    code = reference_polar_code(64, 32)
    with pytest.raises(NpdError):
        code.sc_decode_new(torch.zeros(4, 64), 1.0)
    with pytest.raises(NpdError):
        code.scl_decode(torch.zeros(4, 64), 1.0, 4)
    with pytest.raises(NpdError):
        errors_bler(torch.zeros(4, 8), torch.zeros(4, 8))


def test_list_prune_select_host_utility_matches_std_nth_element(oracle):
    """npd_list_prune_select (the tie rule compiled into the SCL kernel) == std::nth_element (oracle)."""
    import ctypes
    import numpy as np
    from neural_polar_decoder_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(3)
    m = ctypes.c_uint32()
    for n in range(1, 17):
        for k in range(1, n + 1):
            for _ in range(60):
                v = (-rng.integers(0, 3, n)).astype(np.float32)
                assert L.npd_list_prune_select(v.ctypes.data_as(ctypes.c_void_p), n, k, ctypes.byref(m)) == 0
                got = {i for i in range(n) if (m.value >> i) & 1}
                assert got == set(oracle.topk_select(v, k).tolist()), (n, k, v)
    assert L.npd_list_prune_select(None, 4, 2, ctypes.byref(m)) < 0
    v = np.zeros(20, np.float32)
    assert L.npd_list_prune_select(v.ctypes.data_as(ctypes.c_void_p), 20, 2, ctypes.byref(m)) < 0


def test_every_entry_point_rejects_null_operands():
    """Every compute and create entry point, called with NULL for each pointer (handles, operands, out-handles) and
    small valid sizes, returns a negative status with a message -- checked before any HIP call, so it runs without a
    GPU; destroy(NULL) is a no-op.  Run in a child process, so a crash fails this test instead of the session."""
    script = r'''
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from neural_polar_decoder_amd import _lib
L = _lib.load()
skip = {"npd_abi_version", "npd_last_error", "npd_device_count", "npd_conv_workspace_bytes",
        "npd_code_destroy", "npd_gru_destroy", "npd_conv_destroy"}
bad = []
for name, res, argt in _lib.SIGNATURES:
    if name in skip:
        continue
    args = []
    for t in argt:
        if t in (ctypes.c_int, ctypes.c_uint):
            args.append(16)
        elif t in (ctypes.c_long, ctypes.c_ulong):
            args.append(16)
        elif t is ctypes.c_float:
            args.append(1.0)
        else:
            args.append(None)
    rc = getattr(L, name)(*args)
    if not (rc < 0 and L.npd_last_error()):
        bad.append((name, rc))
for d in ("npd_code_destroy", "npd_gru_destroy", "npd_conv_destroy"):
    if getattr(L, d)(None) != 0:
        bad.append((d, "destroy(NULL)"))
print("BAD", bad)
sys.exit(1 if bad else 0)
'''
    r = subprocess.run([os.sys.executable, "-c", script, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
