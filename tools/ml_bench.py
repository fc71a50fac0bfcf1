"""ML / bitwise-MAP decoding throughput on cuda:0 against the baseline a user has today on the same card.

    python tools/ml_bench.py [--out FILE.json] [--quick]

Configurations: Polar(32,16) and PAC(32,10) at B = 2^18, Polar(64,22) at B = 2^12, 2 dB.  Per configuration, after
two warm-up calls, SAMPLES timed windows (device events around enough back-to-back calls to last >= 0.1 s each); the
median window gives the time per call.  Reported:
  * codewords/s of npd_ml_decode (idx only) and npd_map_decode (decisions + LLRs; K <= 16);
  * algorithmic FLOP/s = 2 N 2^K per word, issued = three times that (three fp16 planes; MAP sweeps the codebook
    twice, so six times), each as a fraction of the fp16 dense MFMA peak (2.5 PFLOP/s, the card's spec figure);
  * the torch baseline: (y @ codebook.T).argmax(1) in fp32 on the same card, the codebook (2^K, N) resident, the batch
    chunked so that a chunk's correlations fit in 1 GiB (timed on a sub-batch; its rate does not depend on B).
The ML indices are compared with the baseline's on the baseline's sub-batch (they may differ only on fp32 near-ties).
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import neural_polar_decoder_amd as npd  # noqa: E402
from neural_polar_decoder_amd import _lib  # noqa: E402
from neural_polar_decoder_amd.codes import codebook_masks, generator_rows, masks_to_pm1  # noqa: E402
from neural_polar_decoder_amd.utils import llr_scale  # noqa: E402

PEAK_FP16 = 2.5e15
SAMPLES = 5
SNR = 2.0


def time_call(fn):
    """seconds per call: median of SAMPLES event-timed windows of >= 0.1 s after two warm-up calls"""
    fn(); fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); fn(); e.record()
    torch.cuda.synchronize()
    reps = max(1, int(np.ceil(100.0 / max(s.elapsed_time(e), 1e-3))))
    win = []
    for _ in range(SAMPLES):
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        win.append(s.elapsed_time(e) * 1e-3 / reps)
    return statistics.median(win), min(win), max(win), reps


def bench(kind, N, K, g, B, Bbase):
    dev = torch.device("cuda:0")
    if kind == "pac":
        code = npd.PAC(None, N, K, g)
        h, info = code._code_for(code.B), code.B
    else:
        code = npd.reference_polar_code(N, K)
        h, info = code.code, code.info_positions
    _, _, y = code.mc_generate(B, SNR, seed=1, device=dev, want_msg=False)
    L = _lib.load()
    st = _lib.stream_of(dev)
    idx = torch.empty(B, dtype=torch.int32, device=dev)
    rec = {"code": f"{kind}({N},{K})", "B": B, "snr_db": SNR}

    def ml():
        _lib.check(L.npd_ml_decode(h.h, _lib.ptr(y), None, _lib.ptr(idx), None, B, st), "npd_ml_decode")
    t, lo, hi, reps = time_call(ml)
    alg = 2.0 * N * 2 ** K * B
    rec["ml"] = {"s_per_call": t, "min": lo, "max": hi, "calls_per_window": reps, "cw_per_s": B / t,
                 "algorithmic_flops": alg / t, "issued_flops": 3 * alg / t,
                 "algorithmic_frac_fp16_peak": alg / t / PEAK_FP16, "issued_frac_fp16_peak": 3 * alg / t / PEAK_FP16}
    if code.ml_supported(map=True):
        hat = torch.empty(B, K, device=dev)
        llr = torch.empty(B, K, device=dev)

        def bmap():
            _lib.check(L.npd_map_decode(h.h, _lib.ptr(y), llr_scale(SNR), _lib.ptr(hat), _lib.ptr(llr), B, st),
                       "npd_map_decode")
        t, lo, hi, reps = time_call(bmap)
        rec["map"] = {"s_per_call": t, "min": lo, "max": hi, "calls_per_window": reps, "cw_per_s": B / t,
                      "algorithmic_flops": alg / t, "issued_flops": 6 * alg / t,
                      "algorithmic_frac_fp16_peak": alg / t / PEAK_FP16, "issued_frac_fp16_peak": 6 * alg / t / PEAK_FP16}
    # torch baseline on the first Bbase words
    rows = generator_rows(N, info, g)
    cbT = torch.empty(N, 2 ** K, dtype=torch.float32, device=dev)
    for lo_i in range(0, 2 ** K, 2 ** 18):
        blk = masks_to_pm1(codebook_masks(rows, lo_i, min(2 ** K, lo_i + 2 ** 18)), N, np.float32)
        cbT[:, lo_i:lo_i + blk.shape[0]] = torch.from_numpy(blk).to(dev).T
    chunk = max(1, min(Bbase, (1 << 30) // (4 * 2 ** K)))
    yb = y[:Bbase]
    bidx = torch.empty(Bbase, dtype=torch.int64, device=dev)

    def base():
        for o in range(0, Bbase, chunk):
            bidx[o:o + chunk] = (yb[o:o + chunk] @ cbT).argmax(1)
    t, lo, hi, reps = time_call(base)
    agree = float((bidx == idx[:Bbase].long()).float().mean())
    rec["torch_fp32_baseline"] = {"B": Bbase, "chunk": chunk, "s_per_call": t, "min": lo, "max": hi,
                                  "calls_per_window": reps, "cw_per_s": Bbase / t, "index_agreement": agree}
    rec["ml_speedup_over_torch"] = rec["ml"]["cw_per_s"] / rec["torch_fp32_baseline"]["cw_per_s"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="1/16 of the batches (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ml_bench needs the GPU: there is no CPU path to time")
    q = 16 if a.quick else 1
    out = []
    for kind, N, K, g, B, Bbase in [("polar", 32, 16, 0, 1 << 18, 1 << 15), ("pac", 32, 10, 53, 1 << 18, 1 << 18),
                                    ("polar", 64, 22, 0, 1 << 12, 1 << 9)]:
        rec = bench(kind, N, K, g, B // q, max(64, Bbase // q))
        out.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
