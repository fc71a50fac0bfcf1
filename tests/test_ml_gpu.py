"""GPU: npd_ml_decode / npd_map_decode (csrc/npd_ml.hip) against the reference's ML index and bitwise_MAP decisions
(tests/golden/ml_*.npz, gen_ml.py) and against float64.

Bounds (from the arithmetic, not from the kernel's results):
  eps(y)   = 2 N 2^-24 sum_j |y_j|       two fp32-accumulated sums of N exact products, any order
  delta(y) = 2 [(N + 4) 2^-24 sum_j |a_j| + (2^(K-1) + 8) 2^-24],  a = llr_scale * y
             correlation error + exp2 argument rounding; an fp32 sum of 2^(K-1) positive terms with a 4-ulp exp
"""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

FIXTURES = ["ml_polar_8_2", "ml_polar_16_8", "ml_polar_32_16", "ml_polar_64_12", "ml_pac_32_10", "ml_pac_16_5"]
U = 2.0 ** -24
DEV = "cuda"
_cache = {}


def eps_of(y, N):
    return 2.0 * N * U * np.abs(np.asarray(y, np.float64)).sum(1)


def delta_of(a, N, K):
    return 2.0 * ((N + 4) * U * np.abs(a).sum(1) + (2.0 ** (K - 1) + 8) * U)


def make_code(N, K, info, g=0):
    import neural_polar_decoder_amd as npd
    if g:
        code = npd.PAC(None, N, K, g)
        code.B = np.asarray(info, np.int64)
        return code, code._code_for(code.B)
    code = npd.PolarCode(int(np.log2(N)), K, F=np.setdiff1d(np.arange(N), info))
    return code, code.code


def fixture(name):
    """(fixture, code, handle, float64 codebook (2^K, N)) -- loaded and built once, shared, never modified."""
    if name not in _cache:
        from neural_polar_decoder_amd.codes import codebook_masks, generator_rows, masks_to_pm1
        d = golden(name + ".npz")
        N, K, g = int(d["N"]), int(d["K"]), int(d["g"]) if int(d["pac"]) else 0
        code, h = make_code(N, K, d["info"], g)
        cb = masks_to_pm1(codebook_masks(generator_rows(N, d["info"], g)), N)
        cb.setflags(write=False)
        _cache[name] = (d, code, h, cb)
    return _cache[name]


def ml(h, y, **kw):
    from neural_polar_decoder_amd.polar import ml_decode
    out = ml_decode(h, torch.as_tensor(y, device=DEV), return_idx=True, return_metric=True, **kw)
    return [o.cpu().numpy() for o in out]


# ------------------------------------------------------------------------------------------- 1. golden parity
@pytest.mark.parametrize("name", FIXTURES)
def test_golden_parity(name):
    from neural_polar_decoder_amd.codes import all_message_bits
    d, code, h, cb = fixture(name)
    N, K = int(d["N"]), int(d["K"])
    hat, idx, metric = ml(h, d["y"])
    assert np.array_equal(idx, d["idx"])                       # every word, no exclusions
    assert np.array_equal(hat, all_message_bits(K)[idx])
    corr = (d["y"].astype(np.float64) * cb[idx]).sum(1)
    err = np.abs(metric.astype(np.float64) - corr)
    print(name, "max metric error / (eps/2):", float((err / (eps_of(d["y"], N) / 2)).max()))
    assert np.all(err <= eps_of(d["y"], N) / 2)
    # the public methods return the same decisions
    m2, i2 = code.ml_decode(torch.from_numpy(d["y"]), return_idx=True)       # host input: staged, result comes home
    assert not m2.is_cuda and np.array_equal(i2.numpy(), idx) and np.array_equal(m2.numpy(), hat)


# ------------------------------------------------------------------------------------------- 2. near-optimality
@pytest.mark.parametrize("kind,N,K,g,B", [("polar", 16, 8, 0, 8192), ("polar", 32, 16, 0, 512), ("pac", 32, 10, 53, 512)])
def test_near_optimal_on_unfiltered_words(kind, N, K, g, B):
    from neural_polar_decoder_amd.codes import (codebook_masks, generator_rows, masks_to_pm1, pac_info_positions,
                                                polar_info_positions)
    info = pac_info_positions(N, K, "RM") if g else polar_info_positions(N, K)
    code, h = make_code(N, K, info, g)
    _, _, y = code.mc_generate(B, 0.0, seed=31, device=DEV)
    _, idx, _ = ml(h, y)
    y64 = y.cpu().numpy().astype(np.float64)
    cb = masks_to_pm1(codebook_masks(generator_rows(N, info, g)), N)
    worst = 0.0
    for o in range(0, B, 128):
        corr = y64[o:o + 128] @ cb.T
        chosen = corr[np.arange(corr.shape[0]), idx[o:o + 128]]
        gap = corr.max(1) - chosen
        worst = max(worst, float((gap / eps_of(y64[o:o + 128], N)).max()))
        assert np.all(gap <= eps_of(y64[o:o + 128], N))        # every word
    print(kind, N, K, "worst (best - chosen) / eps:", worst)


# ------------------------------------------------------------------------------------------- 3. exact ties
@pytest.mark.parametrize("name", FIXTURES)
def test_exact_ties_pick_the_smallest_index(name):
    d, code, h, cb = fixture(name)
    N, K = int(d["N"]), int(d["K"])
    rng = np.random.default_rng(5)
    y = rng.integers(-2, 3, size=(256, N)).astype(np.float32)
    y[0] = 0.0                                                  # every codeword ties: index 0
    i, j = rng.integers(0, 2 ** K, size=(2, 64))
    y[1:65] = cb[i] + cb[j]                                     # equidistant from c_i and c_j (and often more)
    y[65:97] = cb[rng.integers(0, 2 ** K, size=32)] * 2.0       # a codeword itself
    y[97:129, N // 2:] = 0.0                                    # half the positions erased
    corr = y.astype(np.int64) @ cb.astype(np.int64).T           # exact
    want = corr.argmax(1)                                       # numpy: the first maximum
    assert (np.sort(corr, 1)[:, -1] == np.sort(corr, 1)[:, -2]).sum() >= 32       # the batch does hold ties
    _, idx, metric = ml(h, y)
    assert idx[0] == 0
    assert np.array_equal(idx, want)
    assert np.array_equal(metric, corr.max(1).astype(np.float32))


# ------------------------------------------------------------------------------------------- 4. shapes and edges
@pytest.mark.parametrize("name", ["ml_polar_8_2", "ml_polar_32_16", "ml_polar_64_12", "ml_pac_16_5"])
def test_batch_sizes_scaling_and_single_outputs(name):
    from neural_polar_decoder_amd import _lib
    d, code, h, cb = fixture(name)
    N, K = int(d["N"]), int(d["K"])
    y = np.concatenate([d["y"], d["y"][:64] * 0.5])             # 256 words
    hat, idx, metric = ml(h, y)
    for B in (1, 15, 17, 255):
        hb, ib, mb = ml(h, y[:B])
        assert np.array_equal(ib, idx[:B]) and np.array_equal(hb, hat[:B]) and np.array_equal(mb, metric[:B])
    off = np.concatenate([np.zeros(3, np.float32), y.ravel()])  # an unaligned base pointer
    _, io, _ = ml(h, torch.as_tensor(off, device=DEV)[3:].view(-1, N))
    assert np.array_equal(io, idx)
    for k in (-12, 10):
        hs, i_s, ms = ml(h, y * np.float32(2.0 ** k))
        assert np.array_equal(i_s, idx) and np.all(np.isfinite(ms)) and np.all(np.isfinite(hs))
        assert np.array_equal(ms, metric * np.float32(2.0 ** k))
    L = _lib.load()
    yt = torch.as_tensor(y, device=DEV)
    st = _lib.stream_of(yt.device)
    o_hat = torch.empty(256, K, device=DEV)
    o_idx = torch.empty(256, dtype=torch.int32, device=DEV)
    o_met = torch.empty(256, device=DEV)
    assert L.npd_ml_decode(h.h, _lib.ptr(yt), _lib.ptr(o_hat), None, None, 256, st) == 0
    assert L.npd_ml_decode(h.h, _lib.ptr(yt), None, _lib.ptr(o_idx), None, 256, st) == 0
    assert L.npd_ml_decode(h.h, _lib.ptr(yt), None, None, _lib.ptr(o_met), 256, st) == 0
    assert np.array_equal(o_hat.cpu().numpy(), hat) and np.array_equal(o_idx.cpu().numpy(), idx)
    assert np.array_equal(o_met.cpu().numpy(), metric)
    assert L.npd_ml_decode(h.h, _lib.ptr(yt), None, _lib.ptr(o_idx), None, 0, st) == 0


@pytest.mark.parametrize("name", ["ml_polar_16_8", "ml_polar_64_12"])
def test_large_batches_take_the_wider_word_tiles(name):
    """npd_ml_decode gives a workgroup 2 or 4 word tiles once the batch fills the card (2^15 / 2^16 words on 256
    CUs): each row of a tiled batch must equal the same word decoded in a small batch (one tile per workgroup).  MAP
    keeps one tile per workgroup; its large batch checks the grid indexing."""
    d, code, h, cb = fixture(name)
    y = torch.as_tensor(d["y"], device=DEV)
    hat, idx, metric = ml(h, y)
    dec, llr = code.bitwise_MAP(y[:64], DEV, 0.0, return_llr=True)
    for B in (2 ** 15 + 5, 2 ** 16 + 2 ** 15 + 17):
        reps = -(-B // y.shape[0])
        yb = y.repeat(reps, 1)[:B].contiguous()
        hb, ib, mb = ml(h, yb)
        assert np.array_equal(ib, np.tile(idx, reps)[:B]) and np.array_equal(mb, np.tile(metric, reps)[:B])
        assert np.array_equal(hb, np.tile(hat, (reps, 1))[:B])
    B = 2 ** 15 + 5                                             # MAP: a batch of many workgroups
    reps = -(-B // 64)
    db, lb = code.bitwise_MAP(y[:64].repeat(reps, 1)[:B].contiguous(), DEV, 0.0, return_llr=True)
    assert torch.equal(lb, llr.repeat(reps, 1)[:B]) and torch.equal(db, dec.repeat(reps, 1)[:B])


def test_polar_64_22_against_a_chunked_float64_argmax():
    from neural_polar_decoder_amd.codes import codebook_masks, generator_rows, polar_info_positions
    N, K = 64, 22
    info = polar_info_positions(N, K)
    code, h = make_code(N, K, info)
    _, _, y = code.mc_generate(8, 1.0, seed=77, device=DEV)
    _, idx, _ = ml(h, y)
    y64 = y.cpu().numpy().astype(np.float64)
    rows = generator_rows(N, info)
    best = np.full(8, -np.inf)
    chosen = np.zeros(8)
    for lo in range(0, 2 ** K, 2 ** 18):
        masks = codebook_masks(rows, lo, lo + 2 ** 18)
        bits = np.unpackbits(masks.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
        corr = (1.0 - 2.0 * bits) @ y64.T                       # (2^18, 8)
        best = np.maximum(best, corr.max(0))
        for b in np.nonzero((idx >= lo) & (idx < lo + 2 ** 18))[0]:
            chosen[b] = corr[idx[b] - lo, b]
    print("(64,22) (best - chosen) / eps:", ((best - chosen) / eps_of(y64, N)).max())
    assert np.all(chosen >= best - eps_of(y64, N))


# ------------------------------------------------------------------------------------------- 5. bitwise MAP
@pytest.mark.parametrize("name", FIXTURES)
def test_bitwise_map_llrs_and_decisions(name):
    d, code, h, cb = fixture(name)
    N, K = int(d["N"]), int(d["K"])
    worst = 0.0
    for si, snr in enumerate((0.0, 2.0, 4.0)):
        rows = slice(64 * si, 64 * si + 64)
        y = d["y"][rows]
        assert np.all(d["snr"][rows] == snr)
        dec, llr = code.bitwise_MAP(torch.as_tensor(y, device=DEV), DEV, snr, return_llr=True)
        dec, llr = dec.cpu().numpy(), llr.cpu().numpy().astype(np.float64)
        a = np.float64(d["scale"][si]) * y.astype(np.float64)
        delta = delta_of(a, N, K)[:, None]
        err = np.abs(llr - d["llr64"][rows])
        worst = max(worst, float(err.max()))
        assert np.all(err <= delta), (snr, float(err.max()), float(delta.min()))   # every bit of every word
        far = np.abs(d["llr64"][rows]) > delta
        assert far.mean() >= 0.99
        ref = d["map_dec"][rows].astype(np.float32) if "map_dec" in d.files else np.where(d["llr64"][rows] >= 0, 1.0, -1.0)
        assert np.array_equal(dec[far], ref[far])
        assert np.array_equal(dec, np.where(llr >= 0, 1.0, -1.0))
        assert np.array_equal(code.bitwise_MAP(torch.as_tensor(y, device=DEV), DEV, snr).cpu().numpy(), dec)
    print(name, "max |llr - LLR64|:", worst, " reference fp32:", float(d["ref_llr_err"]))
    dec8, llr8 = code.bitwise_MAP(torch.as_tensor(d["y"][128:] * 8.0, device=DEV), DEV, 4.0, return_llr=True)
    assert torch.isfinite(llr8).all() and torch.isfinite(dec8).all()


# ------------------------------------------------------------------------------------------- 6. Monte-Carlo, CLI
def test_ml_montecarlo_counts_equal_decode_plus_host_count():
    import neural_polar_decoder_amd as npd
    from neural_polar_decoder_amd.montecarlo import MAPMonteCarlo, MLMonteCarlo
    code = npd.reference_polar_code(32, 16)
    snrs, n = [1.0, 3.0], 1 << 14
    res = MLMonteCarlo(code, snrs, n, n, seed=9).run()
    resm = MAPMonteCarlo(code, snrs, n, n, seed=9).run()
    for si, snr in enumerate(snrs):
        msg, _, y = code.mc_generate(n, snr, 9, si, 0, device=DEV)
        wrong = (code.ml_decode(y) != msg).cpu().numpy()
        assert res.bit_errors[si] == int(wrong.sum()) and res.block_errors[si] == int(wrong.any(1).sum())
        wrong = (code.bitwise_MAP(y, DEV, snr) != msg).cpu().numpy()
        assert resm.bit_errors[si] == int(wrong.sum()) and resm.block_errors[si] == int(wrong.any(1).sum())
    assert res.block_errors[0] > res.block_errors[1] > 0
    with pytest.raises(ValueError):
        MLMonteCarlo(npd.reference_polar_code(128, 16), snrs, n, n)


def test_cli_prints_the_reference_lines(capsys):
    from neural_polar_decoder_amd.montecarlo import _main
    _main(["--N", "32", "--K", "16", "--ml", "--bitwise_map", "--test_size", "4096", "--batch_size", "4096",
           "--snr_points", "2"])
    out = capsys.readouterr().out
    for line in ("BERs of ML:", "BLERs of ML:", "BERs of bitML:", "BLERs of bitML:"):
        assert line in out
    rec = json.loads(out.strip().splitlines()[-1])
    assert rec["ml"]["codewords"] == 4096 and rec["bitwise_map"]["K"] == 16
    assert 0 < rec["ml"]["block_errors"][0] < 4096 and len(rec["bitwise_map"]["ber"]) == 2
    with pytest.raises(SystemExit):
        _main(["--N", "128", "--K", "16", "--ml", "--test_size", "64", "--batch_size", "64", "--snr_points", "1"])


# ------------------------------------------------------------------------------------------- 7. graph capture
def test_ml_decode_under_graph_capture():
    from neural_polar_decoder_amd import _lib
    d, code, h, cb = fixture("ml_polar_32_16")
    L = _lib.load()
    y = torch.as_tensor(d["y"], device=DEV)
    B = y.shape[0]
    idx = torch.zeros(B, dtype=torch.int32, device=DEV)
    met = torch.zeros(B, device=DEV)
    eager_i, eager_m = idx.clone(), met.clone()
    assert L.npd_ml_decode(h.h, _lib.ptr(y), None, _lib.ptr(eager_i), _lib.ptr(eager_m), B, _lib.stream_of(y.device)) == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                   # one kernel node: nothing allocates or synchronises
        rc = L.npd_ml_decode(h.h, _lib.ptr(y), None, _lib.ptr(idx), _lib.ptr(met), B, _lib.stream_of(y.device))
    assert rc == 0
    assert int(idx.abs().sum()) == 0                            # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager_i) and torch.equal(met, eager_m)
    assert np.array_equal(idx.cpu().numpy(), d["idx"])
