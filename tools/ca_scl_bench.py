"""CRC-aided SC-List throughput (codewords/s) on cuda:0 beside plain SC-List on the same words, and its error rates:

    python tools/ca_scl_bench.py [--shapes N:K:g:c:L,...] [--bler] [--out FILE]

Times scl_decode_crc_mc (decode, CRC selection and fused counting, one launch) against scl_decode_mc (the same list
decoder with the distance step: the yardstick) on the same received words, in one process, the two alternating.  Every
shape is warmed up, each timed window lasts at least --window seconds, and every shape is timed --repeats times; the
line carries every rate, the medians' ratio and the spread (max / min - 1 of each decoder's repeats).  g = 0 is a Polar
code (the reference's information set), otherwise the PAC polynomial.

--bler: block errors and crc_fail of Polar(64,32) CRC-8 at L = 8 and L = 32 over 0 .. 4 dB, 2^16 words per point
(CASCLMonteCarlo), with plain SC-List at the same (N, K) and L beside it (SCLMonteCarlo).  One JSON line each."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from neural_polar_decoder_amd import PAC, reference_polar_code  # noqa: E402
from neural_polar_decoder_amd.montecarlo import CASCLMonteCarlo, SCLMonteCarlo  # noqa: E402

#          N    K   g   c  L
SHAPES = [(64, 32, 0, 8, 4), (64, 32, 0, 8, 8), (64, 32, 0, 8, 32), (128, 64, 0, 16, 4), (128, 64, 0, 16, 16),
          (256, 128, 0, 24, 4), (64, 32, 91, 8, 4), (128, 64, 91, 16, 4)]


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / iters


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="least duration of a timed window, seconds")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=None, help="N:K:g:c:L tuples, comma-separated (default: the DESIGN.md rows)")
    ap.add_argument("--snr", type=float, default=2.0)
    ap.add_argument("--bler", action="store_true", help="also the Polar(64,32) CRC-8 error-rate rows")
    ap.add_argument("--no_time", action="store_true", help="skip the throughput rows")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    assert torch.cuda.is_available(), "needs the MI355X"
    shapes = SHAPES
    if a.shapes:
        shapes = [tuple(int(x) for x in t.split(":")) for t in a.shapes.split(",")]
    for N, K, g, c, L in ([] if a.no_time else shapes):
        code = PAC(None, N, K, g) if g else reference_polar_code(N, K)
        code.set_crc(c)
        B = (1 << 18 if N <= 64 else 1 << 16) // (4 if L > 8 else 1)
        y = code.mc_generate_crc(B, a.snr, seed=1, device=dev, want_msg=False)[2]
        cnt = torch.zeros(3, dtype=torch.int64, device=dev)
        fns = {"ca_scl": lambda: code.scl_decode_crc_mc(y, a.snr, L, 1, 0, cnt),
               "scl": lambda: code.scl_decode_mc(y, a.snr, L, 1, 0, cnt[:2])}
        iters = {}
        for k, fn in fns.items():  # warm-up, and the iteration count that fills the window
            window(fn, 2)
            iters[k] = max(3, int(a.window / window(fn, 3)) + 1)
        rates = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k, fn in fns.items():
                rates[k].append(B / window(fn, iters[k]))
        med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
        rec = {"N": N, "K": K, "g": g, "crc_len": c, "L": L, "B": B, "snr": a.snr}
        rec.update({f"{k}_cw_per_s": [round(r) for r in v] for k, v in rates.items()})
        rec.update({f"{k}_spread": round(max(v) / min(v) - 1, 4) for k, v in rates.items()})
        rec["ca_scl_over_scl"] = round(med["ca_scl"] / med["scl"], 4)
        emit(rec, a.out)
    if a.bler:
        snrs = [0.0, 1.0, 2.0, 3.0, 4.0]
        for L in (8, 32):
            code = reference_polar_code(64, 32)
            plain = SCLMonteCarlo(code, L, snrs, 1 << 16, 1 << 16, seed=11).run()
            code.set_crc(8)
            drv = CASCLMonteCarlo(code, L, snrs, 1 << 16, 1 << 16, seed=11)
            ca = drv.run()
            emit({"N": 64, "K": 32, "crc_len": 8, "L": L, "snr": snrs, "codewords": 1 << 16,
                  "ca_scl_block_errors": ca.block_errors, "ca_scl_crc_fail": drv.crc_fail, "ca_scl_K": ca.K,
                  "scl_block_errors": plain.block_errors, "scl_K": plain.K}, a.out)


if __name__ == "__main__":
    main()
