"""SC-List throughput sweep (codewords/s, decode + fused counting in one launch) on cuda:0:

    python tools/scl_bench.py [--Ls 1,2,4,8] [--shapes 64:32,256:128,128:64] [--window 0.3] [--repeats 3] [--out FILE]

Device events; every (shape, L) is warmed up, each timed window lasts at least --window seconds and is repeated
--repeats times, the list sizes alternating within a shape.  One JSON line per (shape, L); when 8 is among the list
sizes, lines of L > 8 also carry `l8_scaled`, the L = 8 rate of the same run times 8 / L (the line a decoder whose
work grew linearly with L would hold), and `over_l8_scaled`.  --Ls 8,16,32 --shapes 64:32,64:22,128:64,256:128 gives
the wide-list rows of DESIGN.md."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from neural_polar_decoder_amd import reference_polar_code  # noqa: E402

SNR = {64: 2.0, 128: 1.0, 256: 1.0}


def window(code, y, snr, L, cnt, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        code.scl_decode_mc(y, snr, L, 1, 0, cnt)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / iters


def sweep(code, N, K, B, snr, Ls, a, tag):
    dev = "cuda:0"
    _, _, y = code.mc_generate(B, snr, seed=1, device=dev, want_msg=False)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    iters = {}
    for L in Ls:  # warm-up, and the iteration count that fills the window
        window(code, y, snr, L, cnt, 1)
        iters[L] = max(2, int(a.window / window(code, y, snr, L, cnt, 2)) + 1)
    rates = {L: [] for L in Ls}
    for _ in range(a.repeats):
        for L in Ls:
            rates[L].append(B / window(code, y, snr, L, cnt, iters[L]))
    med = {L: sorted(v)[len(v) // 2] for L, v in rates.items()}
    for L in Ls:
        rec = {"code": tag, "N": N, "K": K, "L": L, "B": B, "snr": snr, "cw_per_s": [round(r) for r in rates[L]],
               "median": round(med[L])}
        if L > 8 and 8 in med:
            rec["l8_scaled"] = round(med[8] * 8 / L)
            rec["over_l8_scaled"] = round(med[L] / (med[8] * 8 / L), 4)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Ls", default="1,2,4,8", help="list sizes, comma-separated (1 .. 32)")
    ap.add_argument("--shapes", default="64:32,256:128,128:64", help="N:K pairs, comma-separated")
    ap.add_argument("--window", type=float, default=0.3, help="least duration of a timed window, seconds")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    Ls = [int(x) for x in a.Ls.split(",")]
    for nk in a.shapes.split(","):
        N, K = (int(x) for x in nk.split(":"))
        B = 1 << 18 if N <= 64 else 1 << 16
        sweep(reference_polar_code(N, K), N, K, B, SNR.get(N, 2.0), Ls, a, "polar")


if __name__ == "__main__":
    main()
