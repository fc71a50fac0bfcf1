"""GRU list decoding throughput on cuda:0 (npd_gru_list_decode) beside the greedy decoder and a torch restatement.

    python tools/rnnl_bench.py [--case f64|f512] [--out FILE.json] [--quick]

Two configurations, one per run, both seeded 2-layer GRUs (onehot y_input), fp32, at 2 dB, list sizes L = 1, 2, 4, 8:
  f64   Polar(64,32), hidden 64 (gru_list_kernel, weights in LDS), B = 2^18 words, torch on 2^14;
  f512  Polar(64,22), hidden 512 (gru_wide_list_kernel, weights streamed; the CRISP recipe's shape), B = 2^15 words,
        torch on 2^13.
After two warm-up calls every leg is timed with device events around single calls, REPS times;
reported are the median, the minimum and the maximum.  In the same run, on the same words:
  * greedy: RNN_decoder.decode's kernel (npd_gru_decode, fp32).  A wave of the list kernel holds 1 / Lp as many
    codewords (Lp = L rounded up to 1, 2, 4, 8), so the expectation is list time ~ Lp x greedy time; the ratio
    list / (Lp x greedy) is printed per L.
  * torch: the list loop of rnn_all.py:580-664 restated with this package's RNN_Model on the GPU (all live paths of all
    words as one batch per step, topk + sort + gather for the pruning), on fewer words (above) -- what a user has
    without the kernel.
Rates: codewords/s; FLOP/s = 2 x (N (9 F^2) + 3 F N) MACs per path and word (the three GRU GEMMs per step and the y
projection; L = 1 counts one path, the list kernel computes Lp) over the median time, as a fraction of the fp32 MFMA
peak (157.3 TFLOP/s, the spec figure at 2.4 GHz).  The held clock is sampled with `rocm-smi --showclocks` while the L = 8
leg runs (read-only; "not measured" when the tool is not there).
"""
import argparse
import json
import re
import statistics
import subprocess
import sys
import threading

import numpy as np
import torch

sys.path.insert(0, ".")
import neural_polar_decoder_amd as npd  # noqa: E402
from neural_polar_decoder_amd.montecarlo import seeded_crisp  # noqa: E402
from neural_polar_decoder_amd.rnn import get_onehot  # noqa: E402

PEAK_FP32 = 157.3e12
REPS = 10
SNR = 2.0
CASES = {  # name: (N, K, F, layers, log2 B, log2 B of the torch leg)
    "f64": (64, 32, 64, 2, 18, 14),
    "f512": (64, 22, 512, 2, 15, 13),
}
N, K, F, LAYERS = CASES["f64"][:4]


def time_call(fn, reps=REPS):
    """seconds per call: (median, min, max) of `reps` event-timed calls after two warm-up calls"""
    fn(); fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        torch.cuda.synchronize()
        t.append(s.elapsed_time(e) * 1e-3)
    return statistics.median(t), min(t), max(t)


def torch_list_decode(net, y, info, code, L):
    """rnn_all.py:580-664 with the live paths batched: hidden (layers, ls * B, F), one net step per position."""
    B = y.shape[0]
    isinfo = torch.zeros(N, dtype=torch.bool)
    isinfo[torch.as_tensor(info)] = True
    rows = torch.arange(B, device=y.device)
    with torch.no_grad():
        hid = torch.zeros(LAYERS, 1, B, F, device=y.device)
        dec = torch.ones(1, B, N, device=y.device)
        met = torch.zeros(1, B, device=y.device)
        for ii in range(N):
            ls = dec.shape[0]
            prev = torch.ones(ls * B, device=y.device) if ii == 0 else dec[:, :, ii - 1].reshape(-1).sign()
            x = torch.cat([y.repeat(ls, 1), get_onehot(prev)], 1).unsqueeze(1)
            out, h = net(x, hid.reshape(LAYERS, ls * B, F).contiguous())
            out = out.view(ls, B)
            hid = h.view(LAYERS, ls, B, F)
            if not bool(isinfo[ii]):
                continue
            hid = torch.cat([hid, hid], 1)
            dec = torch.cat([dec, dec], 0)
            dec[:ls, :, ii] = out.sign()
            dec[ls:, :, ii] = -out.sign()
            met = torch.cat([met, met + out.abs()], 0)
            if 2 * ls > L:
                keep = torch.topk(-met, L, 0)[1].sort(0)[0]
                hid = hid[:, keep, rows]
                met = met[keep, rows]
                dec = dec[keep, rows]
        ls = dec.shape[0]
        cand = dec[:, :, torch.as_tensor(info, device=y.device)]
        cwd = code.encode_plotkin(cand.reshape(ls * B, K)).reshape(ls, B, N)
        sel = ((cwd - y.unsqueeze(0)) ** 2).sum(2).argmin(0)
        return cand[sel, rows]


class ClockSampler(threading.Thread):
    """sclk samples (MHz) from `rocm-smi --showclocks` while a leg runs; read-only"""

    def __init__(self):
        super().__init__(daemon=True)
        self.stop = threading.Event()
        self.mhz = []

    def run(self):
        while not self.stop.is_set() and len(self.mhz) < 50:
            try:
                txt = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True,
                                     timeout=20).stdout
            except Exception:
                return
            m = re.search(r"sclk clock level:\s*\d+:?\s*\((\d+)Mhz\)", txt)
            if m:
                self.mhz.append(int(m.group(1)))
            self.stop.wait(0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=list(CASES), default="f64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="1/16 of the batches (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnnl_bench needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    global N, K, F, LAYERS
    N, K, F, LAYERS, lb, lbt = CASES[a.case]
    q = 16 if a.quick else 1
    B, Bt = (1 << lb) // q, (1 << lbt) // q
    code = npd.reference_polar_code(N, K)
    info = np.sort(np.asarray(code.info_positions))
    net, dec = seeded_crisp(code, F, LAYERS, seed=0, device=dev)
    _, _, y = code.mc_generate(B, SNR, seed=1, device=dev, want_msg=False)
    flop_path = 2.0 * (N * 9 * F * F + 3 * F * N)
    rec = {"case": a.case, "code": f"polar({N},{K})", "F": F, "layers": LAYERS, "B": B, "snr_db": SNR, "reps": REPS}

    tg, lo, hi = time_call(lambda: dec.decode(net, False, y))
    rec["greedy"] = {"s_per_call": tg, "min": lo, "max": hi, "cw_per_s": B / tg,
                     "frac_fp32_peak": flop_path * B / tg / PEAK_FP32}
    print(json.dumps({"greedy": rec["greedy"]}), flush=True)
    yt = y[:Bt].contiguous()
    for L in (1, 2, 4, 8):
        Lp = 1 if L == 1 else 2 if L == 2 else 4 if L <= 4 else 8
        sampler = ClockSampler() if L == 8 else None
        if sampler:
            sampler.start()
        t, lo, hi = time_call(lambda: dec.list_decode(net, y, code, L))
        if sampler:
            sampler.stop.set()
            sampler.join()
            rec["held_sclk_mhz"] = (statistics.median(sampler.mhz) if sampler.mhz else "not measured")
        tt, tlo, thi = time_call(lambda: torch_list_decode(net, yt, info, code, L), reps=max(3, REPS // 3))
        same = float((torch_list_decode(net, yt, info, code, L) == dec.list_decode(net, yt, code, L)).all(1).float().mean())
        r = {"L": L, "Lp": Lp, "s_per_call": t, "min": lo, "max": hi, "cw_per_s": B / t,
             "frac_fp32_peak": flop_path * Lp * B / t / PEAK_FP32, "over_greedy": t / tg, "over_Lp_greedy": t / (Lp * tg),
             "torch": {"B": Bt, "s_per_call": tt, "min": tlo, "max": thi, "cw_per_s": Bt / tt, "rows_identical": same},
             "speedup_over_torch": (B / t) / (Bt / tt)}
        rec[f"L{L}"] = r
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
