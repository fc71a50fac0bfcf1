"""PAC SC-List throughput (codewords/s) on cuda:0 beside the Polar SC-List kernel at the same (N, K, L):

    python tools/pac_scl_bench.py [--Ls 1,2,4,8] [--shapes 32:16:53,64:22:91,128:64:91] [--out FILE]

Times scl_decode_mc (decode + fused counting, one launch) with device events for
  pac          the PAC code (RM rate profile),
  polar        the reference Polar code of the same (N, K) (its own information set: the yardstick), and
  polar_rm     the Polar kernel on the PAC code's information set (same schedule of forks and path copies as `pac`,
               so the ratio pac / polar_rm is the cost of the PAC leaf rule alone).
Every shape is warmed up, each timed window lasts at least --window seconds, and every shape is timed --repeats
times, the three decoders alternating, so that the spread shows beside the ratios.  One JSON line per shape and list
size (1 .. 32; --Ls 8,16,32 --shapes 64:32:91,64:22:91,128:64:91,256:128:91 gives the wide-list rows of DESIGN.md;
lines of L > 8 then also carry the L = 8 PAC rate of the same run times 8 / L as `pac_l8_scaled`)."""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from neural_polar_decoder_amd import PAC, PolarCode, reference_polar_code  # noqa: E402

SHAPES = [(32, 16, 53, 1 << 18, 2.0), (64, 22, 91, 1 << 18, 1.0), (128, 64, 91, 1 << 16, 2.0)]


def window(code, y, snr, L, cnt, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        code.scl_decode_mc(y, snr, L, 1, 0, cnt)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="least duration of a timed window, seconds")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--Ls", default="1,2,4,8", help="list sizes, comma-separated (1 .. 32)")
    ap.add_argument("--shapes", default=None, help="N:K:g triples, comma-separated (default: the three PAC shapes)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    assert torch.cuda.is_available(), "needs the MI355X"
    shapes = SHAPES
    if a.shapes:
        shapes = [(N, K, g, 1 << 18 if N <= 64 else 1 << 16, 2.0 if N != 64 or K != 22 else 1.0)
                  for N, K, g in (tuple(int(x) for x in t.split(":")) for t in a.shapes.split(","))]
    l8 = None
    for N, K, g, B, snr in shapes:
        pac = PAC(None, N, K, g)
        codes = {"pac": pac, "polar": reference_polar_code(N, K),
                 "polar_rm": PolarCode(int(np.log2(N)), K, F=np.setdiff1d(np.arange(N), pac.B))}
        ys = {k: c.mc_generate(B, snr, seed=1, device=dev, want_msg=False)[2] for k, c in codes.items()}
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        for L in [int(x) for x in a.Ls.split(",")]:
            iters = {}
            for k, c in codes.items():  # warm-up, and the iteration count that fills the window
                window(c, ys[k], snr, L, cnt, 2)
                iters[k] = max(3, int(a.window / window(c, ys[k], snr, L, cnt, 3)) + 1)
            rates = {k: [] for k in codes}
            for _ in range(a.repeats):
                for k, c in codes.items():
                    rates[k].append(B / window(c, ys[k], snr, L, cnt, iters[k]))
            med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
            rec = {"N": N, "K": K, "g": g, "L": L, "B": B, "snr": snr}
            rec.update({f"{k}_cw_per_s": [round(r) for r in v] for k, v in rates.items()})
            rec["pac_over_polar"] = round(med["pac"] / med["polar"], 4)
            rec["pac_over_polar_rm"] = round(med["pac"] / med["polar_rm"], 4)
            if L == 8:
                l8 = (N, K, med["pac"])
            if L > 8 and l8 is not None and l8[:2] == (N, K):
                rec["pac_l8_scaled"] = round(l8[2] * 8 / L)
                rec["pac_over_l8_scaled"] = round(med["pac"] / (l8[2] * 8 / L), 4)
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
