"""CRISP GRU training steps/s on cuda:0: the fused kernels (RNN_decoder.decode(net, True, ...) + backward) beside torch.

    python tools/train_bench.py [--out FILE.json] [--quick]

Per shape -- Polar(64,32) with hidden 64 x 2 layers, and Polar(32,16) with hidden 64 x 2 layers -- at batch 4096, one
step = forward + MSE on the information positions + backward (no optimiser step: it is the same on every path).  After
3 warm-up steps each path is timed with device events around single steps, 20 times; reported is the median.  Paths:
  fused teacher / fused student   npd_gru_train_forward / _backward
  nn.GRU teacher                  the one-call teacher-forcing restatement (tests/golden/train_crisp_gpu.teacher_forced)
  torch student loop              the reference's student-forcing loop (rnn_all.py:485-494) on the GPU: N single-step
                                  net calls and autograd's replay of them -- what the reference itself does on a GPU
Also printed, per shape and mode: the fused path's logit and gradient errors against the float64 restatement
(tests/train_helper.py) forced along the kernel's path on 256 words, beside E_ref (torch's fp32 autograd on the CPU).
Nothing is asserted.  The held clock is sampled with `rocm-smi --showclocks` (read-only) during the fused legs.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import neural_polar_decoder_amd as npd  # noqa: E402
from neural_polar_decoder_amd.montecarlo import seeded_crisp  # noqa: E402
from neural_polar_decoder_amd.rnn import get_onehot  # noqa: E402

SHAPES = [(64, 32, 64, 2), (32, 16, 64, 2)]  # N, K, F, layers
SNR = 1.0


def time_step(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        torch.cuda.synchronize()
        t.append(s.elapsed_time(e) * 1e-3)
    return statistics.median(t), min(t), max(t)


def torch_student(net, y, info_set, N):
    """rnn_all.py:485-494 (y_input, onehot, natural order)."""
    B = y.shape[0]
    decoded = torch.ones(B, N, device=y.device)
    hidden = torch.zeros(net.num_rnn_layers, B, net.feature_size, device=y.device)
    for ii in range(N):
        prev = torch.ones(B, device=y.device) if ii == 0 else decoded[:, ii - 1].sign()
        x = torch.cat([y.unsqueeze(1), get_onehot(prev).view(-1, 1, 2).detach().clone()], 2)
        out, hidden = net(x, hidden)
        if ii in info_set:
            decoded[:, ii] = out.squeeze()
    return decoded


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


def errors(net, dec, code, info, N, F, layers, student, dev):
    import train_helper as T
    _, _, y = code.mc_generate(256, SNR, seed=5, device=dev)
    y = y.cpu().numpy()
    _, gt = T.make_words(256, N, 11)
    gout = np.random.default_rng(12).standard_normal((256, N)).astype(np.float32)
    net.zero_grad()
    out, bits = dec.decode(net, True, torch.from_numpy(y).to(dev), torch.from_numpy(gt).to(dev), 0.0 if student else 1.0,
                           return_path=True)
    (out * torch.from_numpy(gout).to(dev)).sum().backward()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}
    sd = T.state_dict_np(net)
    bits = bits.cpu().numpy()
    w = T.writes_of(N, info, student)
    d64, _, g64 = T.train64(sd, y, gt, layers, True, info, student, False, gout, bits=bits)
    eref = T.e_ref(sd, F, layers, N, True, y, bits, w, gout, g64)
    net.zero_grad()
    return {"logit_err": float(np.abs(out.detach().cpu().numpy() - d64).max()), "grad_err": T.grad_err(grads, g64),
            "E_ref": eref}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="batch 512 and 5 timed steps (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_bench needs the GPU: there is no CPU path to time")
    from train_crisp_gpu import teacher_forced
    dev = torch.device("cuda:0")
    B, reps = (512, 5) if a.quick else (4096, 20)
    rec = {"batch": B, "reps": reps, "snr_db": SNR, "shapes": []}
    for N, K, F, layers in SHAPES:
        code = npd.reference_polar_code(N, K)
        info = np.sort(np.asarray(code.info_positions))
        info_t = torch.as_tensor(info, device=dev)
        info_set = set(info.tolist())
        net, dec = seeded_crisp(code, F, layers, seed=0, device=dev)
        net.train()
        msg, _, y = code.mc_generate(B, SNR, seed=1, device=dev)
        gt = torch.ones(B, N, device=dev)
        gt[:, info_t] = msg
        loss_fn = torch.nn.MSELoss()

        def step(forward):
            net.zero_grad(set_to_none=True)
            loss_fn(forward()[:, info_t], msg).backward()

        legs = {
            "fused_teacher": lambda: step(lambda: dec.decode(net, True, y, gt, 1.0)),
            "fused_student": lambda: step(lambda: dec.decode(net, True, y, gt, 0.0)),
            "nn_gru_teacher": lambda: step(lambda: teacher_forced(net, y, gt)),
            "torch_student_loop": lambda: step(lambda: torch_student(net, y, info_set, N)),
        }
        r = {"code": f"polar({N},{K})", "F": F, "layers": layers}
        sampler = ClockSampler()
        sampler.start()
        for name in ("fused_teacher", "fused_student"):
            t, lo, hi = time_step(legs[name], reps)
            r[name] = {"s_per_step": t, "min": lo, "max": hi, "steps_per_s": 1.0 / t}
        sampler.stop.set()
        sampler.join()
        r["held_sclk_mhz"] = statistics.median(sampler.mhz) if sampler.mhz else "not measured"
        for name in ("nn_gru_teacher", "torch_student_loop"):
            t, lo, hi = time_step(legs[name], reps)
            r[name] = {"s_per_step": t, "min": lo, "max": hi, "steps_per_s": 1.0 / t}
        r["teacher_fused_over_nn_gru"] = r["nn_gru_teacher"]["s_per_step"] / r["fused_teacher"]["s_per_step"]
        r["student_fused_over_torch_loop"] = r["torch_student_loop"]["s_per_step"] / r["fused_student"]["s_per_step"]
        r["errors_teacher"] = errors(net, dec, code, info, N, F, layers, False, dev)
        r["errors_student"] = errors(net, dec, code, info, N, F, layers, True, dev)
        rec["shapes"].append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
