"""convNet training steps/s on cuda:0: the fused kernels (convNet.forward in training mode + backward) beside torch.

    python tools/conv_train_bench.py [--out FILE.json] [--quick]

Shapes: run_alt.sh's (N 64, embed 128, batch 8192) and embed 16 at the same N and batch.  One step = forward + MSE on
the 22 information positions + backward (no optimiser step: it is the same on every path), dropout 0.1 on every path.
Paths:
  fused         npd_conv_train_forward / _backward through convNet.forward
  im2col        tests/golden/train_conv_gpu.ConvNetT: each Conv1d as one GEMM over the im2col of its 7 taps
  conv1d        the same module with native = True: F.conv1d (MIOpen)
After 3 warm-up steps of every path the paths alternate, one step each, 20 rounds, every step between two device events;
reported per path: median, min, max.  The baseline is the faster torch path of this run.  Also reported: the fraction
of the derived 8 ms floor (1.28 TFLOP per step at run_alt.sh's shape over the 155 TF fp32 MFMA rate; scaled by the
layer shapes' FLOPs for the other shape) the fused step reaches.  The held clock is sampled with `rocm-smi
--showclocks` (read-only) while the rounds run.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import threading
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from neural_polar_decoder_amd.models import convNet  # noqa: E402
from neural_polar_decoder_amd.train_conv import plotkin, stage_info  # noqa: E402

SHAPES = [(64, 128), (64, 16)]  # N, embed
PEAK = 155e12


def step_flops(N, E, B):
    """Forward multiply-adds x 2 of the conv and Linear layers; a step is forward + dX + dW = 3 x that (layer 0 has no dX)."""
    h = E // 2
    conv = 7 * (1 * h + 7 * h * h + h * E + E * E) * N
    fc = E * N * 4 * N + 4 * N * N + N * N
    return 3 * 2.0 * B * (conv + fc)


class ClockSampler(threading.Thread):
    """sclk samples (MHz) from `rocm-smi --showclocks` while the rounds run; read-only"""

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
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="batch 512 and 5 rounds (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_train_bench needs the GPU: there is no CPU path to time")
    from train_conv_gpu import ConvNetT
    dev = torch.device("cuda:0")
    B, reps = (512, 5) if a.quick else (8192, 20)
    rec = {"batch": B, "rounds": reps, "dropout": 0.1, "shapes": []}
    for N, E in SHAPES:
        torch.manual_seed(0)
        cfg = types.SimpleNamespace(embed_dim=E, max_len=N, N=N, dont_use_bias=False, dropout=0.1)
        net = convNet(cfg).to(dev).train()
        tnet = ConvNetT(E, N).to(dev).train()
        tnet.load_state_dict(net.state_dict())
        info = torch.as_tensor(stage_info(N, 22, 22), device=dev)
        msg = 1 - 2 * (torch.rand(B, 22, device=dev) < 0.5).float()
        gt = torch.ones(B, N, device=dev)
        gt[:, info] = msg
        y = plotkin(gt) + torch.randn(B, N, device=dev)
        mask = torch.ones(B, N, device=dev).long()
        loss_fn = torch.nn.MSELoss()

        def fused():
            net.zero_grad(set_to_none=True)
            loss_fn(net(y, mask, gt, dev)[3][:, info, 0], msg).backward()

        def torch_step(native):
            tnet.native = native
            tnet.zero_grad(set_to_none=True)
            loss_fn(tnet(y)[:, info], msg).backward()

        legs = {"fused": fused, "im2col": lambda: torch_step(False), "conv1d": lambda: torch_step(True)}
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        sampler = ClockSampler()
        sampler.start()
        for _ in range(reps):
            for name, fn in legs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) * 1e-3)
        sampler.stop.set()
        sampler.join()
        r = {"N": N, "embed": E, "held_sclk_mhz": statistics.median(sampler.mhz) if sampler.mhz else "not measured"}
        for name, t in times.items():
            med = statistics.median(t)
            r[name] = {"s_per_step": med, "min": min(t), "max": max(t), "steps_per_s": 1.0 / med}
        base = min(("im2col", "conv1d"), key=lambda k: r[k]["s_per_step"])
        floor = step_flops(N, E, B) / PEAK
        r.update(baseline=base, fused_over_baseline=r[base]["s_per_step"] / r["fused"]["s_per_step"],
                 floor_s=floor, fused_fraction_of_floor=floor / r["fused"]["s_per_step"])
        rec["shapes"].append(r)
        print(json.dumps(r), flush=True)
        del net, tnet
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
