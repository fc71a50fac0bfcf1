#!/usr/bin/env python3
"""Headline benchmark: the metric BASELINE.json names -- codewords/s of the Polar(64,32) SC + CRISP-GRU eval step
(rnn_all.py:853-880: SC and the CRISP GRU decode the same received words at every SNR point, both counted).

``value`` -- one "step" = for the SNR sweep 0,1,2,3,4 dB, B = 2^20 received words per SNR point per GPU (resident in
HBM before timing): one SC launch over the whole sweep (npd_sc_decode_mc_sweep: decode + fused BER/BLER counts,
msg_hat written) and, per SNR point, one CRISP GRU decode (hidden 64, 2 layers, onehot y_input; the trained
tests/golden/trained_crisp_64_32.npz weights; fp16x3 split MFMA kernel gru16p_kernel, fp32 accumulation) plus its
device error count.  K steps are timed between barrier + synchronize; HIP events on the launch stream time every SC
and GRU launch inside the timed region (the roofline's launch durations).

A plain run does only that: set up, warm up, time the K steps, write --dump-outputs if asked, print the result line.
Everything below runs behind --full.

Other configurations run as sub-records under --full (same weak-scaling rules; every leg decodes its own codeword shard per rank,
timed between barriers, max over ranks; whole-job codewords/s):
  configs1_sc     configs[1]: SC decode alone (the SC half of the step, HBM-bound) + its PMC traffic
  montecarlo      the fused Monte-Carlo step: Philox message -> encode -> AWGN -> SC -> count, y never stored
  crisp_gru       configs[2]: GRU decode alone, fp32 kernel (the reference's arithmetic) + split-MFMA kernels
  crisp_gru_f512  run_crisp.sh's decoder width (hidden 512, weight-streaming kernel)
  pac_gru/pac_sc  configs[3]: PAC(128,64) CRISP GRU and PAC SC, RCCL all-reduce of the counters
  conv_model      configs[4]: Polar(256,128) convNet (embed 128), fp16x3 split MFMA (fp32 path beside)
  scl, sc_lse     SC-List (run_models.py:329) and exact-LSE SC (polar.py:209-279)

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
  --gpus N > 1 without a launcher: bench.py starts `python -m torch.distributed.run --nproc-per-node N`
  on itself (the parent never touches the GPU) and exits with its status.  Under a launcher,
  WORLD_SIZE must equal --gpus.

Rank 0 prints ONE compact JSON line last: the headline and the roofline of its timed launches.  With --full it also
writes the full record (every leg) to --full-json, and the line carries the PMC traffic, cpu_baseline, the comparison
with the reference's curve and one summary per configuration.  cpu_baseline times the CPU oracle (oracle/: C
restatements of sc_decode_new and RNN_decoder.decode) on a bounded sample of the same received words.

--dump-outputs DIR: after the timed steps rank 0 writes what the timed step's caller holds after the last step as
DIR/<name>.npy (dump_outputs below).  The inputs are Philox words and fixture weights, identical from run to run.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_CODE, K_CODE = 64, 32
BYTES_PER_CW = 4 * N_CODE + 4 * K_CODE  # y in + msg_hat out
HBM_PEAK_GBS = 8000.0                    # MI355X spec (MI355X_MICROARCH.md); 6.3 TB/s measured copy
FP32_PEAK_TF = 157.3                     # MI355X fp32 vector / fp32 MFMA (MI355X_MICROARCH.md)
FP16_PEAK_TF = 2516.6                    # MI355X dense fp16 / bf16 MFMA (MI355X_MICROARCH.md)
SEED = 1234
# the reference's own sc_decode_new curve (tests/golden/sc_anchors_64_32.npz: 2e5 words at 0-1 dB, 1e6 at 2-4 dB)
ANCHORS_NPZ = os.path.join(ROOT, "tests", "golden", "sc_anchors_64_32.npz")


def db_offsets(snrs, bler, ref_snrs, ref_bler):
    """Horizontal offset (dB) of a BLER curve from the reference's: the SNR at which the reference's log-BLER
    (linear between grid points, end segments extended) equals log(bler), minus the point's SNR."""
    rs = np.asarray(ref_snrs, float)
    lr = np.log(np.maximum(np.asarray(ref_bler, float), 1e-300))
    out = []
    for s_, p in zip(snrs, bler):
        if p <= 0:
            out.append(None)
            continue
        lp = np.log(p)
        j = next((i for i in range(len(rs) - 1) if (lr[i] - lp) * (lr[i + 1] - lp) <= 0 and lr[i] != lr[i + 1]), None)
        if j is None:
            j = 0 if abs(lp - lr[0]) < abs(lp - lr[-1]) else len(rs) - 2
        out.append(float(rs[j] + (lp - lr[j]) / (lr[j + 1] - lr[j]) * (rs[j + 1] - rs[j]) - s_))
    return out


def gru_flop_per_cw(N, F):
    """y.W_ih once + per step the two layers' gate GEMVs and the output dot."""
    return 2 * 3 * F * N + N * (2 * 3 * F * F + 2 * 2 * 3 * F * F + 2 * F)


TRAINED_64_32 = os.path.join(ROOT, "tests", "golden", "trained_crisp_64_32.npz")
TRAINED_PAC = os.path.join(ROOT, "tests", "golden", "trained_pac_128_64.npz")  # none trained yet


def trained_or_seeded(code, path, info, dev, precision="fp32"):
    """A CRISP GRU (hidden 64, 2 layers, onehot y_input): the trained fixture at `path` (tests/golden/gen_trained.py:
    curriculum stages on the GPU, final stage by the reference's own training loop) when present, else PyTorch-default
    seeded weights.  Returns (net, decoder, description, fixture or None)."""
    from neural_polar_decoder_amd.montecarlo import seeded_crisp
    from neural_polar_decoder_amd.rnn import RNN_Model, RNN_decoder
    if os.path.exists(path):
        d = np.load(path)
        N, F = int(d["N"]), int(d["F"])
        net = RNN_Model("GRU", N + 2, F, 1, int(d["layers"]), N, 0, 0).to(dev).eval()
        net.load_state_dict({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w.")})
        if not np.array_equal(d["info"], np.asarray(info)):
            raise SystemExit(f"{path}: trained CRISP fixture is for another information set")
        dec = RNN_decoder("y_input", N, np.asarray(info), onehot=True, precision=precision)
        return net, dec, f"trained (tests/golden/{os.path.basename(path)})", d
    net, dec = seeded_crisp(code, 64, 2, seed=0, device=dev, precision=precision)
    return net, dec, "seeded untrained weights (trained fixture absent)", None


def crisp_model(code, dev, precision="fp32"):
    """The CRISP GRU of configs[2] (Polar(64,32)): trained_or_seeded with the Polar(64,32) fixture."""
    return trained_or_seeded(code, TRAINED_64_32, code.info_positions, dev, precision)


def gru_vs_reference(fix, snrs, bit_err, blk_err, n_cw, K):
    """GRU BER/BLER of this run against the reference's own Monte-Carlo curve for the same trained weights
    (fixture: n words per SNR through RNN_decoder.decode on the CPU): two-sample z of BLER (binomial) and of
    BER (per-codeword bit-error variance from the fixture's sum of squares)."""
    if fix is None:
        return None
    out = {}
    for i, s in enumerate(snrs):
        j = [float(x) for x in fix["snr"]].index(float(s)) if float(s) in [float(x) for x in fix["snr"]] else None
        if j is None:
            continue
        nr = int(fix["mc_n"])
        pr, pb = int(fix["mc_blk_err"][j]) / nr, int(fix["mc_bit_err"][j]) / (nr * K)
        p, b = blk_err[i] / n_cw, bit_err[i] / (n_cw * K)
        pool = (int(fix["mc_blk_err"][j]) + blk_err[i]) / (nr + n_cw)
        zb = (p - pr) / max(1e-300, np.sqrt(pool * (1 - pool) * (1 / nr + 1 / n_cw)))
        ev = int(fix["mc_sq_err"][j]) / nr - (int(fix["mc_bit_err"][j]) / nr) ** 2   # var of bit errors per word
        zr = (b - pb) * K / max(1e-300, np.sqrt(ev * (1 / nr + 1 / n_cw)))
        out[str(s)] = {"ber": b, "ber_reference": pb, "z_ber": zr, "bler": p, "bler_reference": pr, "z_bler": zb}
    out["reference_words_per_snr"] = int(fix["mc_n"])
    out["within_4_sigma"] = bool(all(abs(v["z_ber"]) < 4 and abs(v["z_bler"]) < 4
                                     for k, v in out.items() if isinstance(v, dict)))
    return out


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--snrs", type=str, default="0,1,2,3,4")
    ap.add_argument("--full", action="store_true",
                    help="also run every other configuration, the CPU baselines, the PMC traffic pass and the comparisons "
                         "with the reference (the --no-* switches below trim that); off: the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step to DIR/<name>.npy (rank 0)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="budget of the CPU-baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-gru", action="store_true", help="skip the GRU legs besides the headline (fp32 path, crisp_gru, crisp_gru_f512, pac_gru)")
    ap.add_argument("--no-traffic", action="store_true", help="skip the rocprofv3 PMC traffic pass")
    ap.add_argument("--no-conv", action="store_true", help="skip the conv-model leg")
    ap.add_argument("--no-scl", action="store_true", help="skip the SC-List leg")
    ap.add_argument("--no-lse", action="store_true", help="skip the exact-LSE SC leg")
    ap.add_argument("--no-mc", action="store_true", help="skip the fused Monte-Carlo leg")
    ap.add_argument("--no-pac", action="store_true", help="skip the PAC(128,64) SC leg")
    ap.add_argument("--full-json", default=os.path.join(ROOT, "gpurun_out", "bench_full.json"),
                    help="where rank 0 writes the full record (every leg); the printed line is the compact summary")
    ap.add_argument("--traffic-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launch-probe", action="store_true", help=argparse.SUPPRESS)  # CPU test of the launcher
    return ap.parse_args()


# ------------------------------------------------------------------------------- launch / distributed
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(args):
    """--gpus N > 1 with no launcher: one rank per GPU through torch.distributed.run, as a child process
    (this process has not initialised HIP and never does)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def dist_setup():
    """One rank per GPU over RCCL (backend "nccl").  Rehearsal switches for a box with fewer GPUs than ranks (tested by
    tests/test_bench_launch.py on one MI355X; never used for a reported number): NPD_BENCH_BACKEND=gloo and
    NPD_BENCH_SHARE_GPU=1 (rank r on GPU r mod device count)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        backend = os.environ.get("NPD_BENCH_BACKEND", "nccl")
        dev_index = local
        if os.environ.get("NPD_BENCH_SHARE_GPU") == "1":
            dev_index = local % max(1, torch.cuda.device_count())
        torch.cuda.set_device(dev_index)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend)
        if dist.get_world_size() != world:
            raise SystemExit(f"process-group world size {dist.get_world_size()} != WORLD_SIZE {world}")
    else:
        torch.cuda.set_device(0)
    return world, rank, local


def barrier(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def allreduce(t, op, world):
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(t, op=op)
    return t


def _max():
    import torch.distributed as dist
    return dist.ReduceOp.MAX


def _sum():
    import torch.distributed as dist
    return dist.ReduceOp.SUM


class Timer:
    """Barrier + synchronize on both sides of `iters` calls of fn; seconds per call, max over ranks."""

    def __init__(self, world, dev):
        self.world, self.dev = world, dev

    def __call__(self, fn, iters=1, warm=1):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        barrier(self.world)
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        barrier(self.world)
        el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=self.dev)
        return float(allreduce(el, _max(), self.world).item()) / iters


def event_ms(fn, iters, stream):
    """Average per-call device time of fn by HIP events recorded on the stream the kernels run on."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record(stream)
    for _ in range(iters):
        fn()
    e.record(stream)
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


# ------------------------------------------------------------------------------------ CPU baseline
def available_cores():
    """Cores this process may use: the affinity set, capped by a cgroup CPU quota when one is set."""
    n = len(os.sched_getaffinity(0))
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(-(-int(q) // int(p)))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(ys_host, snrs, info, budget_s):
    """Oracle (bit-exact C restatement of sc_decode_new) on the host cores, timed over repeated passes
    of a bounded sample of the same received words until ~budget_s seconds of CPU work are done."""
    from oracle import oracle as O
    threads = available_cores()
    O.set_num_threads(threads)
    O.sc_decode(ys_host[0][:4096], snrs[0], info)  # warm
    done, passes = 0, 0
    t0 = time.perf_counter()
    while True:
        for s, y in zip(snrs, ys_host):
            O.sc_decode(y, s, info)
            done += y.shape[0]
        passes += 1
        el = time.perf_counter() - t0
        if el >= budget_s:
            break
    import platform
    cpu = platform.processor() or "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"value": done / el, "unit": "codewords/s", "cores": threads, "kind": "port",
            "sample": f"oracle sc_decode (C, OpenMP, {threads} threads = all cores of the affinity set / cgroup "
                      f"quota, {cpu}): {passes} passes over the first {ys_host[0].shape[0]} received words of "
                      f"each of {len(snrs)} SNR points ({done} codewords, {el:.1f} s)",
            "reference_measured_8core": 4.67e3}


# ------------------------------------------------------------------------------------ secondary legs
def mc_leg(code, snrs, B, cw0, world, timer, dev, ref_counts):
    """The Monte-Carlo step: message -> encode -> AWGN -> SC -> count for every SNR point, y never
    stored (npd_sc_mc_sweep_fused).  Counts must equal the decode-only leg's on the same words."""
    cnt = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)

    def step():
        code.sc_mc_sweep_fused(B, snrs, SEED, cw0, cnt)

    step()
    torch.cuda.synchronize()
    one = cnt.clone()
    cnt.zero_()
    t = timer(step, iters=5, warm=1)
    ms = event_ms(step, 3, stream)
    allreduce(one, _sum(), world)
    return {"value": world * len(snrs) * B / t, "unit": "codewords/s", "ms_per_step": t * 1e3,
            "avg_launch_ms": ms, "counts_equal_decode_leg": bool(torch.equal(one.cpu(), ref_counts)),
            "bound": "VALU (Philox + Box-Muller + SC per codeword; no HBM traffic besides counters)",
            "config": "Polar(64,32), 2^20 codewords per SNR per GPU, 0-4 dB, one fused launch per sweep"}


# the GRU precision study (tools/gru_precision.py): the decoding Polar(32,16) net first (round 5), the headline's
# Polar(64,32) net beside it (round 4)
PRECISION_JSONS = {"trained_crisp_32_16 (decoding net)": os.path.join(ROOT, "profiles", "round5", "gru_precision_32_16.json"),
                   "trained_crisp_64_32 (headline net)": os.path.join(ROOT, "profiles", "round4", "gru_precision.json")}


def sc_plus_gru_fp32(code, snrs, B, cw0, world, timer, dev, yall, msg, hat):
    """The headline step with the GRU on the fp32 kernel (gru_decode_kernel<64,2>, the reference's arithmetic):
    the same SC launch and five GRU decodes + counts.  Reported beside the fp16x3 headline."""
    from neural_polar_decoder_amd.utils import count_errors
    c_sc = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
    cg = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)
    net, dec, _, _ = crisp_model(code, dev, precision="fp32")

    def step():
        code.sc_decode_mc_sweep(yall, snrs, SEED, cw0, c_sc, msg_hat=hat)
        for si in range(len(snrs)):
            count_errors(msg, dec.decode(net, False, yall[si]), cg[si], cols=code.info_positions)

    t = timer(step, iters=2, warm=1)
    ms = event_ms(lambda: dec.decode(net, False, yall[2]), 2, stream)
    allreduce(cg, _sum(), world)
    cc = cg.cpu().numpy() // 3  # three counted passes
    tf = gru_flop_per_cw(N_CODE, 64) * B / (ms / 1e3) / 1e12
    n = world * B
    return {"value": world * len(snrs) * B / t, "ms_per_step": t * 1e3,
            "roofline": {"bound": "mfma", "kernel": "gru_decode_kernel<64,2> (fp32 v_mfma_f32_32x32x2_f32)",
                         "achieved": tf, "peak": FP32_PEAK_TF, "unit": "TFLOP/s", "frac": tf / FP32_PEAK_TF,
                         "avg_launch_ms": ms},
            "gru_ber": {str(s_): float(cc[i, 0]) / (n * K_CODE) for i, s_ in enumerate(snrs)},
            "gru_bler": {str(s_): float(cc[i, 1]) / n for i, s_ in enumerate(snrs)}}


def cpu_baseline_sc_gru(yall_host, snrs, info, net, budget_s):
    """The metric-as-named step on the host: the oracle's SC (sc_decode) and GRU (gru_decode) restatements, C with
    OpenMP on every core of the affinity set, decoding the same received words until ~budget_s of CPU work."""
    from oracle import oracle as O
    threads = available_cores()
    O.set_num_threads(threads)
    sd = {k: v.detach().float().cpu().numpy() for k, v in net.state_dict().items()}
    nb = yall_host[0].shape[0]
    O.gru_decode(yall_host[0][:256], sd, N_CODE, 64, 2, info)  # warm
    done, t0 = 0, time.perf_counter()
    while True:
        for s, y in zip(snrs, yall_host):
            O.sc_decode(y, s, info)
            O.gru_decode(y, sd, N_CODE, 64, 2, info)
            done += y.shape[0]
        el = time.perf_counter() - t0
        if el >= budget_s:
            break
    return {"value": done / el, "unit": "codewords/s (each decoded by SC and by the GRU)", "cores": threads,
            "kind": "port", "sample": f"oracle sc_decode + gru_decode (C, OpenMP, {threads} threads): the first {nb} "
                                      f"received words of each of {len(snrs)} SNR points, repeated ({done} codewords, "
                                      f"{el:.1f} s)"}


def gru_leg(code, dev, y, B, world, timer):
    """configs[2]: CRISP GRU hidden 64, 2 layers, Polar(64,32), B = 2^20, fused decode kernel.  The fp32
    kernel (the reference's arithmetic) is the value; the opt-in bf16x3 / bf16 MFMA kernels are timed
    beside it with their decision agreement against fp32 on the same words."""
    flop_cw = gru_flop_per_cw(N_CODE, 64)
    stream = torch.cuda.current_stream(dev)
    res, ref_dec = {}, None
    for prec, peak in (("fp32", FP32_PEAK_TF), ("fp16x3", 2516.6), ("bf16x3", 2516.6), ("bf16", 2516.6)):
        net, dec, wdesc, _ = crisp_model(code, dev, precision=prec)
        d0, l0 = dec.decode(net, False, y, return_logits=True)
        t = timer(lambda: dec.decode(net, False, y), iters=2, warm=0)
        ms = event_ms(lambda: dec.decode(net, False, y), 2, stream)
        tflops = flop_cw * B / (ms / 1e3) / 1e12
        r = {"value": world * B / t, "avg_launch_ms": ms, "achieved_tflops": tflops, "peak_tflops": peak,
             "frac": tflops / peak}
        if ref_dec is None:
            ref_dec, ref_lg = d0, l0
            r["median_abs_logit"] = l0.abs().median().item()
        else:
            same = (d0 == ref_dec).all(1)
            r["cw_agreement_vs_fp32"] = same.float().mean().item()
            dl = (l0[same] - ref_lg[same]).abs()
            r["max_logit_diff_vs_fp32_on_agreeing_cw"] = dl.max().item()
            # relative to max(1, |logit|): trained logits reach O(10-100), where fp32 itself resolves ~1e-5
            r["max_rel_logit_diff_vs_fp32_on_agreeing_cw"] = (dl / ref_lg[same].abs().clamp_min(1.0)).max().item()
        res[prec] = r
    f = res["fp32"]
    return {"value": f["value"], "unit": "codewords/s", "batch_per_gpu": B, "avg_launch_ms": f["avg_launch_ms"],
            "dtype": "fp32 (v_mfma_f32_32x32x2_f32)", "algorithmic_flop_per_cw": flop_cw,
            "achieved_tflops": f["achieved_tflops"], "peak_tflops_fp32": FP32_PEAK_TF, "frac": f["frac"],
            "fp16x3": dict(res["fp16x3"], note="unscaled hi+lo fp16 split with the gate exp2 constants folded into the "
                                                "weights (gru16p_kernel<5>: 3 products per multiply, fp32 accumulate): "
                                                "held to the fp32 path's tolerance in tests/test_gru_gpu.py"),
            "bf16x3": res["bf16x3"], "bf16": res["bf16"], "weights": wdesc,
            "config": "configs[2]: Polar(64,32) CRISP GRU hidden 64, 2 layers, onehot y_input, 2 dB, 2^20 per GPU"}


TRAINED_32_16 = os.path.join(ROOT, "tests", "golden", "trained_crisp_32_16.npz")


def db_bar(snrs, bler, n, ref_bler, nr):
    """The +-0.05 dB bar of tests/test_trained_gru_gpu.py on a BLER curve: per point whose reference BLER is in
    [1e-3, 0.9], the horizontal offset from the reference's curve and its binomial sigma_dB (both samples, over the
    reference's local slope); 'resolvable' where 3 sigma_dB <= 0.05, and there |offset| <= 0.05 must hold."""
    offs = db_offsets(snrs, bler, snrs, ref_bler)
    lr = np.log(np.maximum(ref_bler, 1e-300))
    pts, ok = {}, True
    for i, (s_, o, p, pr) in enumerate(zip(snrs, offs, bler, ref_bler)):
        if not 1e-3 <= pr <= 0.9 or p <= 0:
            continue
        j0, j1 = max(i - 1, 0), min(i + 1, len(snrs) - 1)
        slope = abs(lr[j1] - lr[j0]) / (snrs[j1] - snrs[j0])
        sig = float(np.sqrt((1 - p) / (p * n) + (1 - pr) / (pr * nr)) / max(slope, 1e-9))
        res = 3 * sig <= 0.05
        within = o is not None and (abs(o) <= 0.05 if res else abs(o) <= 3 * sig)
        ok = ok and within
        pts[str(s_)] = {"offset_db": o, "sigma_db": sig, "resolvable": res, "within": within}
    n_res = sum(v["resolvable"] for v in pts.values())
    return {"points": pts, "resolvable_points": n_res, "ber_match_0.05dB": bool(ok and n_res >= 2)}


TRAINED_PAC_32_10 = os.path.join(ROOT, "tests", "golden", "trained_pac_32_10.npz")


def decoding_net_leg(dev, rank, world, timer, B=1 << 20, path=TRAINED_32_16):
    """The headline's GRU kernel (gru16p_kernel<5>, fp16x3, the same fused sweep + count launch) on a net that DECODES:
    tests/golden/trained_crisp_32_16.npz (Polar(32,16) rev_polar CRISP GRU hidden 64, 2 layers; reference BLER 0.73 ->
    0.16 over 0-4 dB, its final stage trained by the reference's rnn_all.py).  2^20 Philox words per SNR per GPU, BER /
    BLER against the reference's own Monte-Carlo curve for the same weights (2^20 words per SNR through
    RNN_decoder.decode on the CPU): z-tests and the +-0.05 dB bar.  The headline net (Polar(64,32) hidden 64) does not
    decode (BLER ~ 1), so this record is where the headline kernel's BER match is measured.  With
    path = tests/golden/trained_pac_32_10.npz the same record for configs[3]'s code family: a PAC(32,10) CRISP GRU
    (g = 53, hidden 64; reference BLER 0.22 -> 0.017 over 0-4 dB) on the same kernel, counted against the PAC message."""
    if not os.path.exists(path):
        return None
    import argparse as _ap
    from neural_polar_decoder_amd import PAC, reference_polar_code
    d = np.load(path)
    N, K = int(d["N"]), int(d["K"])
    if "pac" in d.files and int(d["pac"]) == 1:
        code = PAC(_ap.Namespace(target_K=K), N, K, int(d["g"]) if "g" in d.files else 91)
        info = code.B
    else:
        code = reference_polar_code(N, K)
        info = code.info_positions
    net, dec, wdesc, fix = trained_or_seeded(code, path, info, dev, precision="fp16x3")
    snrs = [float(x) for x in fix["snr"]]
    yall = torch.empty(len(snrs), B, N, dtype=torch.float32, device=dev)
    msg = None
    for si, s_ in enumerate(snrs):
        m, _, _ = code.mc_generate(B, s_, SEED + 1, si, rank * B, want_msg=msg is None, out=yall[si])
        msg = m if msg is None else msg
    c = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
    dec.decode_count_sweep(net, yall, msg, c)  # counted once; the timed passes below count into scratch
    cs = torch.zeros_like(c)
    t = timer(lambda: dec.decode_count_sweep(net, yall, msg, cs), iters=2, warm=1)
    allreduce(c, _sum(), world)
    cc = c.cpu().numpy()
    n = world * B
    nr = int(fix["mc_n"])
    bler = [float(cc[i, 1]) / n for i in range(len(snrs))]
    ref_bler = [int(x) / nr for x in fix["mc_blk_err"]]
    return {"value": world * len(snrs) * B / t, "unit": "codewords/s", "ms_per_sweep": t * 1e3,
            "kernel": "gru16p_kernel<5> (fp16x3, npd_gru_decode_count_sweep: 5 SNR points in one launch)",
            "weights": wdesc, "words_per_snr": n,
            "ber": {str(s_): float(cc[i, 0]) / (n * K) for i, s_ in enumerate(snrs)},
            "bler": {str(s_): b for s_, b in zip(snrs, bler)},
            "bler_reference": {str(s_): b for s_, b in zip(snrs, ref_bler)},
            "gru_vs_reference": gru_vs_reference(fix, snrs, cc[:, 0], cc[:, 1], n, K),
            "db_bar": db_bar(snrs, bler, n, ref_bler, nr),
            "config": f"{'PAC' if isinstance(code, PAC) else 'Polar'}({N},{K}) CRISP GRU hidden 64, 2 layers (trained, "
                      f"decodes), 0-4 dB, 2^20 words per SNR per GPU"}


TRAINED_F512 = os.path.join(ROOT, "tests", "golden", "trained_crisp_64_22_f512.npz")


def crisp_f512_leg(dev, rank, world, timer, B=1 << 15):
    """The CRISP curriculum's decoder (run_crisp.sh): Polar(64,22) rev_polar profile, GRU hidden 512, 2 layers, onehot;
    fp32 weight-streaming MFMA kernel (weights 9.4 MB, read from L2/MALL each step).  Weights: the trained fixture
    (tests/golden/crisp_cases.py trained_crisp_64_22_f512: run_crisp.sh's stage order on the GPU, last stage by the
    reference's rnn_all.py) when present, with its BER/BLER at 0-4 dB against the reference's own curve for the same
    weights; else seeded."""
    import argparse as _ap
    from neural_polar_decoder_amd import PolarCode
    from neural_polar_decoder_amd.codes import polar_info_positions
    info = polar_info_positions(64, 22, "rev_polar", 22)
    code = PolarCode(6, 22, _ap.Namespace(), F=np.setdiff1d(np.arange(64), info))
    fix = None
    if os.path.exists(TRAINED_F512):
        net, dec, wdesc, fix = trained_or_seeded(code, TRAINED_F512, code.info_positions, dev)
    else:
        from neural_polar_decoder_amd.montecarlo import seeded_crisp
        net, dec = seeded_crisp(code, 512, 2, seed=0, device=dev)
        wdesc = "seeded untrained weights"
    _, _, y = code.mc_generate(B, 0.0, SEED, 0, rank * B, device=dev, want_msg=False)
    stream = torch.cuda.current_stream(dev)
    t = timer(lambda: dec.decode(net, False, y), iters=1, warm=1)
    ms = event_ms(lambda: dec.decode(net, False, y), 1, stream)
    flop_cw = gru_flop_per_cw(64, 512)
    tf = flop_cw * B / (ms / 1e3) / 1e12
    out = {"value": world * B / t, "unit": "codewords/s", "batch_per_gpu": B, "avg_launch_ms": ms,
           "algorithmic_flop_per_cw": flop_cw, "achieved_tflops": tf, "peak_tflops_fp32": FP32_PEAK_TF,
           "frac": tf / FP32_PEAK_TF, "dtype": "fp32 (v_mfma_f32_32x32x2_f32)", "weights": wdesc,
           "config": "run_crisp.sh decoder: Polar(64,22) rev_polar, CRISP GRU hidden 512, 2 layers, onehot, 0 dB"}
    if fix is not None:  # the BER curve of the trained decoder against the reference's (2^17 words per SNR there)
        from neural_polar_decoder_amd.utils import count_errors
        snrs = [float(x) for x in fix["snr"]]
        n = 1 << 17
        c = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
        for si, s_ in enumerate(snrs):
            msg, _, ys = code.mc_generate(n, s_, SEED, si, rank * n, device=dev)
            count_errors(msg, dec.decode(net, False, ys), c[si], cols=code.info_positions)
        allreduce(c, _sum(), world)
        cc = c.cpu().numpy()
        out["gru_vs_reference"] = gru_vs_reference(fix, snrs, cc[:, 0], cc[:, 1], world * n, 22)
        ref_bler = [int(x) / int(fix["mc_n"]) for x in fix["mc_blk_err"]]
        bl = [float(cc[i, 1]) / (world * n) for i in range(len(snrs))]
        out["bler_db_offset_vs_reference"] = {str(s_): o for s_, o in zip(snrs, db_offsets(snrs, bl, snrs, ref_bler))}
    return out


def pac_legs(snrs, B, rank, world, timer, dev, do_gru, do_sc):
    """configs[3]: PAC(128,64) (RM profile, g = 91), 2^20 codewords per GPU per SNR (2^23 over 8 GPUs),
    received words resident; CRISP GRU hidden 64 and PAC SC; one RCCL all-reduce of the counters."""
    import argparse as _ap
    from neural_polar_decoder_amd import PAC
    from neural_polar_decoder_amd.utils import count_errors
    code = PAC(_ap.Namespace(target_K=64), 128, 64, 91)
    cw0 = rank * B
    ys, msg = [], None
    for si, snr in enumerate(snrs):
        m, _, y = code.mc_generate(B, snr, SEED, si, cw0, device=dev, want_msg=msg is None)
        msg = m if msg is None else msg
        ys.append(y)
    out = {}
    stream = torch.cuda.current_stream(dev)
    if do_sc:
        c = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
        hat = torch.empty(B, 64, dtype=torch.float32, device=dev)  # decoded message bits, as the eval returns them

        def sc_step():
            for si, snr in enumerate(snrs):
                code.sc_decode_mc(ys[si], snr, SEED, cw0, c[si], msg_hat=hat)

        t = timer(sc_step, iters=3, warm=1)
        ms = event_ms(lambda: code.sc_decode_mc(ys[2], snrs[2], SEED, cw0, c[2], msg_hat=hat), 3, stream)
        c.zero_()
        sc_step()
        allreduce(c, _sum(), world)
        cc = c.cpu().numpy()
        nb = 768 * B  # 4N + 4K bytes per codeword: y in, msg_hat out
        out["pac_sc"] = {"value": world * len(snrs) * B / t, "unit": "codewords/s", "ms_per_step": t * 1e3,
                         "avg_launch_ms": ms, "roofline": {"bound": "hbm", "achieved": nb / (ms / 1e3) / 1e9,
                                                           "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                           "frac": nb / (ms / 1e3) / 1e9 / HBM_PEAK_GBS,
                                                           "algorithmic_bytes_per_launch": nb, "traffic": None},
                         "ber": {str(s): float(cc[i, 0]) / (world * B * 64) for i, s in enumerate(snrs)},
                         "bler": {str(s): float(cc[i, 1]) / (world * B) for i, s in enumerate(snrs)},
                         "config": "PAC(128,64) SC (pac_sc_decode, pac_code.py:534-573), 2^20 per SNR per GPU, 0-4 dB"}
        # the configs[3] eval's SC baseline as its Monte-Carlo step (rnn_all.py:730-776): generation fused into
        # the decode kernel (npd_sc_mc_sweep_fused), y never stored; counts equal the streaming leg's
        cf = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)

        def mc_step():
            code.sc_mc_sweep_fused(B, snrs, SEED, cw0, cf)

        mc_step()
        torch.cuda.synchronize()
        one = cf.clone()
        allreduce(one, _sum(), world)
        tm = timer(mc_step, iters=3, warm=1)
        msm = event_ms(mc_step, 2, stream)
        out["montecarlo_pac"] = {"value": world * len(snrs) * B / tm, "unit": "codewords/s", "ms_per_step": tm * 1e3,
                                 "avg_launch_ms": msm, "counts_equal_streaming_leg": bool(torch.equal(one, c)),
                                 "bound": "latency (serial SC leaf chain + Philox/Box-Muller per codeword; no HBM "
                                          "traffic besides counters)",
                                 "config": "PAC(128,64) fused Monte-Carlo sweep: message -> PAC encode -> AWGN -> SC -> "
                                           "count, 2^20 per SNR per GPU, 0-4 dB, one launch"}
    if do_gru:
        # the record runs the fp16x3 split kernel (its logit error against float64 is the fp32 kernel's on this very
        # net: tests/test_gru_precision_gpu.py[seeded_pac_128_64]); the fp32 kernel's step is reported beside it
        net, dec, wdesc, fix = trained_or_seeded(code, TRAINED_PAC, code.B, dev)
        net16, dec16, _, _ = trained_or_seeded(code, TRAINED_PAC, code.B, dev, precision="fp16x3")
        flop_cw = gru_flop_per_cw(128, 64)
        yall = torch.stack(ys)
        del ys
        res = {}
        for tag, nt, dc in (("fp16x3", net16, dec16), ("fp32", net, dec)):
            c = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
            if tag == "fp16x3":  # the whole sweep in one launch, errors counted in the decision epilogue
                def gru_step():
                    dc.decode_count_sweep(nt, yall, msg, c, cols=code.B)
            else:
                def gru_step():
                    for si in range(len(snrs)):
                        count_errors(msg, dc.decode(nt, False, yall[si]), c[si], cols=code.B)

            dc.decode(nt, False, yall[0][:64])  # weight packing + upload happen here, outside the timed region
            t = timer(gru_step, iters=1, warm=0)
            if tag == "fp16x3":
                cs = torch.zeros_like(c)
                ms = event_ms(lambda: dc.decode_count_sweep(nt, yall, msg, cs, cols=code.B), 1, stream) / len(snrs)
            else:
                ms = event_ms(lambda: dc.decode(nt, False, yall[2]), 1, stream)
            allreduce(c, _sum(), world)  # the RCCL BER reduce of configs[3]
            res[tag] = (t, ms, c.cpu().numpy())
        t, ms16, cc = res["fp16x3"]
        t32, ms, cc32 = res["fp32"]
        n = world * B  # counted once per SNR (the timer's single call); the event pass does not count
        tf = flop_cw * B / (ms / 1e3) / 1e12
        tf16 = flop_cw * B / (ms16 / 1e3) / 1e12
        out["pac_gru"] = {"value": world * len(snrs) * B / t, "unit": "codewords/s", "ms_per_step": t * 1e3,
                          "avg_ms_per_snr_point": ms16, "algorithmic_flop_per_cw": flop_cw, "achieved_tflops": tf16,
                          "peak_tflops_fp16": FP16_PEAK_TF, "frac": tf16 / FP16_PEAK_TF, "issued_frac": 3 * tf16 / FP16_PEAK_TF,
                          "dtype": "fp16x3 (hi + lo fp16 MFMA operands, fp32 accumulation and gates)",
                          "fp32_path": {"value": world * len(snrs) * B / t32, "avg_launch_ms": ms, "achieved_tflops": tf,
                                        "peak_tflops_fp32": FP32_PEAK_TF, "frac": tf / FP32_PEAK_TF,
                                        "counts_equal_fp16x3": bool(np.array_equal(cc, cc32))},
                          "total_codewords": world * len(snrs) * B,
                          "ber": {str(s): float(cc[i, 0]) / (n * 64) for i, s in enumerate(snrs)},
                          "bler": {str(s): float(cc[i, 1]) / n for i, s in enumerate(snrs)},
                          "weights": wdesc,
                          "gru_vs_reference": gru_vs_reference(fix, snrs, cc[:, 0], cc[:, 1], n, 64),
                          "config": "configs[3]: PAC(128,64) CRISP GRU hidden 64, 2 layers, fp16x3 (fp32 beside); 2^20 "
                                    "per SNR per GPU (2^23 at 8 GPUs), 0-4 dB, RCCL counter all-reduce"}
    return out


def scl_leg(code64, dev, y64, snr, world, timer):
    """SC-List: Polar(64,32) L = 4, 8 and Polar(256,128) L = 4 (the C5 eval's per-batch call,
    run_models.py:329); decode + fused counts (npd_scl_decode_mc)."""
    from neural_polar_decoder_amd import reference_polar_code
    stream = torch.cuda.current_stream(dev)
    B = 1 << 18
    yb = y64[:B].contiguous()
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    res = {}
    for L in (4, 8):
        t = timer(lambda: code64.scl_decode_mc(yb, snr, L, SEED, 0, cnt), iters=3, warm=1)
        res[f"N64_L{L}"] = {"value": world * B / t, "avg_launch_ms": event_ms(
            lambda: code64.scl_decode_mc(yb, snr, L, SEED, 0, cnt), 2, stream)}
    c256 = reference_polar_code(256, 128)
    B2 = 1 << 16
    _, _, y2 = c256.mc_generate(B2, 1.0, SEED, 0, 0, device=dev, want_msg=False)
    t = timer(lambda: c256.scl_decode_mc(y2, 1.0, 4, SEED, 0, cnt), iters=2, warm=1)
    res["N256_L4"] = {"value": world * B2 / t, "avg_launch_ms": event_ms(
        lambda: c256.scl_decode_mc(y2, 1.0, 4, SEED, 0, cnt), 2, stream), "batch_per_gpu": B2}
    return {"value": res["N64_L4"]["value"], "unit": "codewords/s", "list_size": 4, "batch_per_gpu": B,
            "avg_launch_ms": res["N64_L4"]["avg_launch_ms"], "L8": res["N64_L8"], "polar_256_128_L4": res["N256_L4"],
            "bound": "latency (profiles/round3/pmc_secondary.json: N=256 L=4 LDS-array busy 0.12 of cycles, VALU issue "
                     "0.085, waves waiting 0.55 of cycles at 1 wave/SIMD; N=64 L=4 LDS 0.35, VALU 0.23)",
            "config": "scl_decode(L) (polar.py:793-876), Polar(64,32) at 2 dB and Polar(256,128) at 1 dB, "
                      "decode + fused BER/BLER counts"}


def lse_leg(code, dev, y, snr, world, timer):
    """exact-LSE SC (PolarCode.sc_decode, polar.py:209-279), Polar(64,32) at 2 dB, hard and soft,
    msg_hat out.  Transcendental-bound (4 exp/log per check node, 192 check nodes per codeword)."""
    B = 1 << 18
    yb = y[:B].contiguous()
    stream = torch.cuda.current_stream(dev)
    res = {}
    for tag, hard in (("hard", True), ("soft", False)):
        t = timer(lambda: code.sc_decode(yb, snr, hard_decision=hard), iters=2, warm=1)
        res[tag] = {"value": world * B / t,
                    "avg_launch_ms": event_ms(lambda: code.sc_decode(yb, snr, hard_decision=hard), 2, stream)}
    return {"value": res["soft"]["value"], "unit": "codewords/s", "batch_per_gpu": B, "soft": res["soft"],
            "hard": res["hard"],
            "bound": "VALU latency (profiles/round3/pmc_secondary.json: VALU issue 0.24-0.27 of peak, 2.0k "
                     "transcendentals of ~15k VALU instructions per codeword, waves waiting 0.5 of cycles at 3 "
                     "waves/SIMD: dependent exp -> log chains)",
            "config": "Polar(64,32) sc_decode exact-LSE (polar.py:209-279), 2 dB, msg_hat out"}


CONV_PRECISION_JSON = os.path.join(ROOT, "profiles", "round5", "conv_precision.json")


def conv_leg(dev, rank, world, timer, batch=8192):
    """configs[4]: Polar(256,128) convNet decoder, embed 128 (run_alt.sh), seeded random weights; batch per GPU,
    whole-job codewords/s.  The record runs the fp16x3 path (conv and Linear layers on v_mfma_f32_32x32x16_f16, hi + lo
    split, fp32 accumulation): measured, its logit error against a float64 forward is below the fp32 path's at every
    percentile (profiles/round5/conv_precision.json, tools/conv_precision.py); tests/test_conv_gpu.py enforces the looser
    bound of 1.5x the fp32 path's error at p50 / p99 / p99.9 and 2x at the maximum; the fp32 MFMA path is reported beside
    it (fp32_path)."""
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.montecarlo import seeded_conv
    net = seeded_conv(256, 128, seed=0, device=dev)
    code = reference_polar_code(256, 128)
    _, _, y = code.mc_generate(batch, 1.0, SEED, 0, rank * batch, device=dev, want_msg=False)
    stream = torch.cuda.current_stream(dev)
    flop_cw = 258.8e6  # 2 x (95.5 M conv + 33.9 M FC) MAC
    res = {}
    for prec in ("fp32", "fp16x3"):
        net.precision = prec
        t = timer(lambda: net.logits(y), iters=3, warm=1)
        ms = event_ms(lambda: net.logits(y), 2, stream)
        lg, _ = net.logits(y[:512])
        res[prec] = dict(t=t, ms=ms, lg=lg, tf=flop_cw * batch / (ms / 1e3) / 1e12)
    net.precision = "fp32"
    p16, p32 = res["fp16x3"], res["fp32"]
    prec_table = json.load(open(CONV_PRECISION_JSON)) if os.path.exists(CONV_PRECISION_JSON) else None
    return {"value": world * batch / p16["t"], "unit": "codewords/s", "batch_per_gpu": batch,
            "avg_forward_ms": p16["ms"],
            "dtype": "fp16x3: conv layers (cin > 1) and Linear layers on v_mfma_f32_32x32x16_f16, hi + lo fp16 split, "
                     "3 products, fp32 accumulation; layer 0, epilogues and LayerNorm fp32",
            "achieved_tflops_fp32_equivalent": p16["tf"],
            "roofline": {"bound": "mfma", "kernel": "conv_ws16_kernel / conv_split_ws_kernel / fc_split_wsp_kernel (fp16x3)",
                         "achieved": 3 * p16["tf"], "unit": "TFLOP/s (fp16 MFMA work issued: 3 products)",
                         "peak": FP16_PEAK_TF, "frac": 3 * p16["tf"] / FP16_PEAK_TF},
            "max_abs_logit_diff_vs_fp32": float((p16["lg"] - p32["lg"]).abs().max()),
            "precision_evidence": None if prec_table is None else {
                "source": "profiles/round5/conv_precision.json (tools/conv_precision.py, final round-5 kernels)",
                "abs_logit_error_vs_float64": {c: {k: {q: v[k][q] for q in ("p50", "p99", "p99.9", "max")}
                                                   for k in ("reference", "fp32", "fp16x3")}
                                               for c, v in prec_table["cases"].items()}},
            "fp32_path": {"value": world * batch / p32["t"], "avg_forward_ms": p32["ms"],
                          "dtype": "fp32 (v_mfma_f32_32x32x2_f32)", "achieved_tflops": p32["tf"],
                          "peak_tflops_fp32": FP32_PEAK_TF, "frac": p32["tf"] / FP32_PEAK_TF},
            "config": "configs[4]: Polar(256,128) convNet embed 128, seeded weights",
            "trained_scaled_down": trained_conv_curve(dev, rank, world, TRAINED_CONV),
            "trained_run_alt_e128": trained_conv_curve(dev, rank, world, TRAINED_CONV_E128)}


TRAINED_CONV = os.path.join(ROOT, "tests", "golden", "trained_conv_64_22.npz")
# round 6: run_alt.sh's own width (embed 128, Polar(64,22) n2c; tests/golden/train_conv_gpu.py + gen_trained_conv.py)
TRAINED_CONV_E128 = os.path.join(ROOT, "tests", "golden", "trained_conv_64_22_e128.npz")


def trained_conv_curve(dev, rank, world, path, n=1 << 18, precision="fp16x3"):
    """A trained conv fixture (embed 16: the reference's run_models.py over run_alt.sh's curriculum shape; embed 128:
    run_alt.sh's width, stages on the GPU): BER/BLER over 0-4 dB on Philox words through the record's fp16x3 kernels,
    against the reference's own Monte-Carlo curve for the same weights, with the +-0.05 dB bar (db_bar)."""
    if not os.path.exists(path):
        return None
    import argparse as _ap
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.models import convNet
    d = np.load(path)
    N, K = int(d["N"]), int(d["K"])
    net = convNet(_ap.Namespace(embed_dim=int(d["embed"]), max_len=N, N=N, dont_use_bias=False, dropout=0.0),
                  precision=precision)
    net.load_state_dict({k[2:]: torch.from_numpy(np.asarray(d[k])) for k in d.files if k.startswith("w.")})
    net.eval()
    code = reference_polar_code(N, K)
    info = torch.as_tensor(d["info"], device=dev)
    snrs = [float(x) for x in d["snr"]]
    c = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
    sq = torch.zeros(len(snrs), dtype=torch.int64, device=dev)
    for si, s_ in enumerate(snrs):
        for off in range(0, n, 1 << 16):
            msg, _, y = code.mc_generate(1 << 16, s_, SEED, si, rank * n + off, device=dev)
            _, dec = net.logits(y)
            e = (dec[:, info] != msg).sum(1).to(torch.int64)
            c[si, 0] += e.sum()
            c[si, 1] += (e > 0).sum()
            sq[si] += (e * e).sum()
    allreduce(c, _sum(), world)
    cc = c.cpu().numpy()
    tot = world * n
    ref_bler = [int(x) / int(d["mc_n"]) for x in d["mc_blk_err"]]
    bler = [float(cc[i, 1]) / tot for i in range(len(snrs))]
    return {"weights": os.path.relpath(path, ROOT), "precision": precision, "embed": int(d["embed"]),
            "words_per_snr": tot, "db_bar": db_bar(snrs, bler, tot, ref_bler, int(d["mc_n"])),
            "ber": {str(s_): float(cc[i, 0]) / (tot * K) for i, s_ in enumerate(snrs)},
            "bler": {str(s_): b for s_, b in zip(snrs, bler)},
            "bler_reference": {str(s_): b for s_, b in zip(snrs, ref_bler)},
            "bler_db_offset_vs_reference": {str(s_): o for s_, o in zip(snrs, db_offsets(snrs, bler, snrs, ref_bler))}}


# ------------------------------------------------------------------------------------ PMC traffic
KERNEL_NAME = "sc_fast_kernel<64>"


def traffic_child(args):
    """Child process under rocprofv3 --pmc: a few decode launches of the timed configuration."""
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    from neural_polar_decoder_amd import reference_polar_code
    code = reference_polar_code(N_CODE, K_CODE)
    B = args.batch
    snrs = [float(s) for s in args.snrs.split(",")]
    yall = torch.empty(len(snrs), B, N_CODE, dtype=torch.float32, device=dev)
    msg = None
    for si, snr in enumerate(snrs):
        m, _, _ = code.mc_generate(B, snr, SEED, si, 0, want_msg=msg is None, out=yall[si])
        msg = m if msg is None else msg
    hat = torch.empty(len(snrs), B, K_CODE, dtype=torch.float32, device=dev)
    cnt = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
    for _ in range(4):
        code.sc_decode_mc_sweep(yall, snrs, SEED, 0, cnt, msg_hat=hat)
    # the headline's GRU launches: fp16x3 CRISP GRU over the whole sweep, errors counted in the kernel
    net, dec, _, _ = crisp_model(code, dev, precision="fp16x3")
    for _ in range(4):
        dec.decode_count_sweep(net, yall, msg, cnt)
    torch.cuda.synchronize()
    del yall, hat
    # the pac_sc leg's launch: PAC(128,64) streaming SC + counts + msg_hat, 2^20 words at 2 dB
    import argparse as _ap
    from neural_polar_decoder_amd import PAC
    pac = PAC(_ap.Namespace(target_K=64), 128, 64, 91)
    _, _, yp = pac.mc_generate(B, 2.0, SEED, 2, 0, device=dev, want_msg=False)
    hp = torch.empty(B, 64, dtype=torch.float32, device=dev)
    for _ in range(4):
        pac.sc_decode_mc(yp, 2.0, SEED, 0, cnt[0], msg_hat=hp)
    torch.cuda.synchronize()


PAC_KERNEL = "sc_decode_kernel<128"
GRU_KERNEL = "gru16p_kernel"


def pmc_traffic(args, timeout_s=240):
    """HBM bytes per launch of the SC decode kernel, the headline's GRU kernel and the pac_sc leg's kernel, from
    rocprofv3 PMC counters, one counter per pass (MI355X_MICROARCH.md 'HBM': FETCH_SIZE reads half the bytes of wide
    coalesced streaming reads on gfx950 -> doubled; WRITE_SIZE exact for 16-B/lane streaming stores; both in KiB).
    Returns ({kernel prefix: bytes per launch}, how)."""
    import csv
    import glob
    import shutil
    import tempfile
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None, "rocprofv3 not found", None
    names = (KERNEL_NAME.split("<")[0], PAC_KERNEL, GRU_KERNEL)
    vals = {k: {} for k in names}
    tmp = tempfile.mkdtemp(prefix="npd_pmc_")
    env = dict(os.environ, TMPDIR="/tmp")
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = os.path.join(tmp, ctr)
        cmd = [prof, "--pmc", ctr, "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
               os.path.abspath(__file__), "--traffic-child", "--batch", str(args.batch), "--snrs", args.snrs]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s, env=env, cwd=ROOT)
        except Exception as e:  # noqa: BLE001
            return None, f"rocprofv3 failed: {e}", None
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None, f"rocprofv3 rc={r.returncode}", None
        rows = list(csv.DictReader(open(files[0])))
        for k in names:
            xs = [float(row["Counter_Value"]) for row in rows if k in row["Kernel_Name"] and row["Counter_Name"] == ctr]
            if not xs:
                return None, f"kernel {k} not found in PMC output", None
            vals[k][ctr] = sum(xs[1:]) / max(1, len(xs) - 1) if len(xs) > 1 else xs[0]  # skip the first (cold) launch
    shutil.rmtree(tmp, ignore_errors=True)
    return ({k: (2 * v["FETCH_SIZE"] + v["WRITE_SIZE"]) * 1024 for k, v in vals.items()},
            "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (x2 read), one pass each",
            {k: {c: v[c] * 1024 for c in v} for k, v in vals.items()})


# ------------------------------------------------------------------------------------ outputs
DUMP_MSG_HAT_BYTES = 32 << 20  # of the 64 MB a dump may take


def dump_outputs(out_dir, hat, c_sc, c_gru):
    """What the caller of the timed step holds after its last step, as float32 / float64 .npy files:
      sc_msg_hat       (n_snr, rows, K) float32  SC's decoded message bits (+-1) of the last step; all B rows when they
                                                 fit DUMP_MSG_HAT_BYTES, else a fixed sample (PCG64(SEED), sorted)
      sc_msg_hat_rows  (rows,) float64           the codeword indices of those rows
      sc_counts        (n_snr, 2) float64        SC [bit errors, block errors], accumulated over the timed steps
      gru_counts       (n_snr, 2) float64        the CRISP GRU's, likewise (its decisions are counted in the kernel's
                                                 epilogue and never stored)"""
    os.makedirs(out_dir, exist_ok=True)
    nsnr, B, K = hat.shape
    rows = min(B, DUMP_MSG_HAT_BYTES // (4 * K * nsnr))
    idx = np.arange(B) if rows == B else np.sort(np.random.default_rng(SEED).choice(B, rows, replace=False))
    sample = hat if rows == B else hat[:, torch.from_numpy(idx).to(hat.device)]
    np.save(os.path.join(out_dir, "sc_msg_hat.npy"), sample.cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "sc_msg_hat_rows.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, "sc_counts.npy"), c_sc.cpu().numpy().astype(np.float64))
    np.save(os.path.join(out_dir, "gru_counts.npy"), c_gru.cpu().numpy().astype(np.float64))


# ------------------------------------------------------------------------------------ main
def sc_only_record(code, snrs, B, cw0, world, dev, yall, hat, steps, warmup):
    """configs[1]: the SC half of the step alone -- one npd_sc_decode_mc_sweep launch per step (decode + fused counts
    + msg_hat) over the resident sweep; K steps between barriers, HIP events per launch (HBM roofline)."""
    counters = torch.zeros(len(snrs), 2, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)
    for _ in range(warmup):
        code.sc_decode_mc_sweep(yall, snrs, SEED, cw0, counters, msg_hat=hat)
    counters.zero_()
    ev = [[torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)] for _ in range(steps)]
    torch.cuda.synchronize()
    barrier(world)
    t0 = time.perf_counter()
    for k in range(steps):
        ev[k][0].record(stream)
        code.sc_decode_mc_sweep(yall, snrs, SEED, cw0, counters, msg_hat=hat)
        ev[k][1].record(stream)
    torch.cuda.synchronize()
    barrier(world)
    el = float(allreduce(torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev), _max(), world))
    launch_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))
    per_step_counts = (counters // steps).cpu()
    allreduce(counters, _sum(), world)
    cnt = counters.cpu().numpy()
    n_cw = steps * world * B
    bler = [float(cnt[i, 1]) / n_cw for i in range(len(snrs))]
    achieved = BYTES_PER_CW * B * len(snrs) / (launch_ms / 1e3) / 1e9
    rec = {"value": world * steps * len(snrs) * B / el, "unit": "codewords/s", "ms_per_step": el / steps * 1e3,
           "roofline": {"bound": "hbm", "kernel": KERNEL_NAME + " (npd_sc_decode_mc_sweep: all SNR points in one launch)",
                        "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                        "traffic": None, "algorithmic_bytes_per_launch": BYTES_PER_CW * B * len(snrs),
                        "avg_launch_ms": launch_ms},
           "ber": {str(s_): float(cnt[i, 0]) / (n_cw * K_CODE) for i, s_ in enumerate(snrs)},
           "bler": {str(s_): b for s_, b in zip(snrs, bler)},
           "config": "configs[1]: Polar(64,32) min-sum SC decode + fused BER/BLER count + msg_hat, 2^20 per SNR per GPU, "
                     "0-4 dB, one launch per sweep"}
    if os.path.exists(ANCHORS_NPZ):  # BER curve vs the reference's: horizontal offset of the BLER curve (+-0.05 dB)
        an = np.load(ANCHORS_NPZ)
        ref_bler = [int(e) / int(n) for e, n in zip(an["blk_err"], an["n"])]
        offs = db_offsets(snrs, bler, [float(x) for x in an["snr"]], ref_bler)
        rec["ber_db_offset"] = {str(s_): o for s_, o in zip(snrs, offs)}
        rec["ber_match"] = all(o is not None and abs(o) <= 0.05 for o in offs)
        rec["ber_reference"] = ("tests/golden/sc_anchors_64_32.npz: the reference's sc_decode_new, 2e5 words at 0-1 dB, "
                                f"1e6 at 2-4 dB; this run: {B} distinct words per SNR")
    return rec, per_step_counts


def main():
    args = parse()
    if args.traffic_child:
        return traffic_child(args)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        return self_launch(args)
    if int(env_world or 1) != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={env_world} ranks", file=sys.stderr)
        return 2
    if args.launch_probe:  # launcher check without a GPU: report the rank layout and stop
        print(json.dumps({"rank": int(os.environ.get("RANK", "0")), "world": int(env_world or 1)}), flush=True)
        return 0
    world, rank, local = dist_setup()
    dev = torch.device("cuda", torch.cuda.current_device())
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.utils import count_errors

    code = reference_polar_code(N_CODE, K_CODE)
    info = code.info_positions
    snrs = [float(s) for s in args.snrs.split(",")]
    nsnr = len(snrs)
    B = args.batch
    cw0 = rank * B  # weak scaling: every rank owns its own codeword range
    # the received words of every SNR point, back to back (n_snr, B, N), resident before timing
    yall = torch.empty(nsnr, B, N_CODE, dtype=torch.float32, device=dev)
    msg = None
    for si, snr in enumerate(snrs):
        m, _, _ = code.mc_generate(B, snr, SEED, si, cw0, want_msg=msg is None, out=yall[si])
        msg = m if msg is None else msg
    ys = [yall[si] for si in range(nsnr)]
    hat = torch.empty(nsnr, B, K_CODE, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)

    # ---------------------------------------------------------------- headline: the SC + CRISP-GRU eval step
    net, dec, wdesc, fix = crisp_model(code, dev, precision="fp16x3")
    # weight packing + upload happen in the first (warm-up) step, outside the timed region
    c_sc = torch.zeros(nsnr, 2, dtype=torch.int64, device=dev)
    c_gru = torch.zeros(nsnr, 2, dtype=torch.int64, device=dev)

    def step(ev=None):
        # decoded_SC_msg_bits and the RNN's decisions on the same words at every SNR point (rnn_all.py:853-880):
        # one SC launch and one GRU launch over the whole sweep, both counting errors in their decision epilogues
        if ev is not None:
            ev[0].record(stream)
        code.sc_decode_mc_sweep(yall, snrs, SEED, cw0, c_sc, msg_hat=hat)
        if ev is not None:
            ev[1].record(stream)
        dec.decode_count_sweep(net, yall, msg, c_gru)
        if ev is not None:
            ev[2].record(stream)

    for _ in range(args.warmup):
        step()
    c_sc.zero_()
    c_gru.zero_()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
    torch.cuda.synchronize()
    barrier(world)
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(ev[k])
    torch.cuda.synchronize()
    barrier(world)
    el = time.perf_counter() - t0
    elapsed = float(allreduce(torch.tensor([el], dtype=torch.float64, device=dev), _max(), world).item())
    rank_ms = [el / args.steps * 1e3]
    if world > 1:
        import torch.distributed as dist
        g = [None] * world
        dist.all_gather_object(g, el / args.steps * 1e3)
        rank_ms = g
    sc_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))
    gru_sweep_ms = float(np.mean([e[1].elapsed_time(e[2]) for e in ev]))
    gru_ms = gru_sweep_ms / nsnr  # per 2^20-codeword SNR point
    if args.dump_outputs and rank == 0:  # this rank's shard, before the counters are summed over ranks
        dump_outputs(args.dump_outputs, hat, c_sc, c_gru)
    allreduce(c_sc, _sum(), world)
    allreduce(c_gru, _sum(), world)
    csc, cg = c_sc.cpu().numpy(), c_gru.cpu().numpy()
    n_cw = args.steps * world * B  # words counted per SNR point
    value = world * args.steps * nsnr * B / elapsed
    flop_cw = gru_flop_per_cw(N_CODE, 64)
    tf16 = flop_cw * B / (gru_ms / 1e3) / 1e12
    sc_gbs = BYTES_PER_CW * B * nsnr / (sc_ms / 1e3) / 1e9
    gru_ber = [float(cg[i, 0]) / (n_cw * K_CODE) for i in range(nsnr)]
    gru_bler = [float(cg[i, 1]) / n_cw for i in range(nsnr)]
    headline = {
        "metric": "codewords/sec Polar(64,32) SC + CRISP-GRU decode, 1/2/4/8 GPU; BER match",
        "value": value, "unit": "codewords/s (each decoded by SC and by the CRISP GRU)",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "fp16x3 GRU (hi+lo fp16 MFMA operands, fp32 accumulate/gates); fp32 SC",
        "data": "synthetic Philox AWGN words, resident in HBM; GRU weights " + wdesc,
        "config": {"workload": "configs[1]+[2]: Polar(64,32) eval step (rnn_all.py:853-880): SC sweep launch + per SNR "
                               "a CRISP GRU decode (hidden 64, 2 layers) + BER/BLER counts, 2^20 words/SNR/GPU, 0-4 dB",
                   "code": "Polar(64,32) 'polar' rate profile", "batch_per_snr_per_gpu": B, "snr_db": snrs,
                   "parallelism": f"dp{world} (codeword shards; one counter all-reduce)"},
        "world_size_rccl": world, "rank_ms_per_step": rank_ms,
        "dist_backend": (os.environ.get("NPD_BENCH_BACKEND", "nccl") if world > 1 else None),
        "roofline": {"bound": "mfma",
                     "kernel": "gru16p_kernel<5> (fp16x3 CRISP GRU: the whole SNR sweep in one launch, errors counted "
                               "in the decision epilogue; npd_gru_decode_count_sweep)",
                     "achieved": tf16, "peak": FP16_PEAK_TF, "unit": "TFLOP/s", "frac": tf16 / FP16_PEAK_TF,
                     "traffic": None,
                     "algorithmic": f"{flop_cw:.4g} FLOP/codeword (SURVEY.md 8(d)) x {nsnr} x {B} codewords per launch",
                     "issued_frac": 3 * tf16 / FP16_PEAK_TF,
                     "issued_note": "3 fp16 products per multiply (hi.hi + hi.lo + lo.hi): the split's redundant "
                                    "products are not useful work, frac (algorithmic) is the roofline fraction",
                     "avg_launch_ms": gru_sweep_ms, "avg_ms_per_snr_point": gru_ms,
                     "step_overhead_ms": elapsed / args.steps * 1e3 - sc_ms - gru_sweep_ms,
                     "sc_launch": {"bound": "hbm", "kernel": KERNEL_NAME, "achieved": sc_gbs, "peak": HBM_PEAK_GBS,
                                   "unit": "GB/s", "frac": sc_gbs / HBM_PEAK_GBS, "avg_launch_ms": sc_ms,
                                   "algorithmic_bytes_per_launch": BYTES_PER_CW * B * nsnr}},
        "gru_ber": {str(s_): b for s_, b in zip(snrs, gru_ber)},
        "gru_bler": {str(s_): b for s_, b in zip(snrs, gru_bler)},
        "sc_ber": {str(s_): float(csc[i, 0]) / (n_cw * K_CODE) for i, s_ in enumerate(snrs)},
        "sc_bler": {str(s_): float(csc[i, 1]) / n_cw for i, s_ in enumerate(snrs)},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(_round_floats(headline)), flush=True)
        return 0
    gvr = gru_vs_reference(fix, snrs, cg[:, 0], cg[:, 1], n_cw, K_CODE)
    full = {"headline": headline, "gru_vs_reference": gvr}
    ev_tabs = {}
    for tag, path in PRECISION_JSONS.items():
        if os.path.exists(path):
            tab = json.load(open(path))
            ev_tabs[tag] = {"source": os.path.relpath(path, ROOT) + " (tools/gru_precision.py)", "words": tab["words"],
                            "abs_logit_error_vs_float64": {k: {q: v[q] for q in ("p50", "p99", "p99.9", "max", "cw_flips")}
                                                           for k, v in tab["impls"].items()}}
    if ev_tabs:
        full["gru_precision_evidence"] = ev_tabs

    timer = Timer(world, dev)
    legs = {}
    sc1, per_step_counts = sc_only_record(code, snrs, B, cw0, world, dev, yall, hat, args.steps, args.warmup)
    legs["configs1_sc"] = sc1
    if not args.no_gru:
        legs["fp32_path"] = sc_plus_gru_fp32(code, snrs, B, cw0, world, timer, dev, yall, msg, hat)
    if not args.no_mc and hasattr(code, "sc_mc_sweep_fused"):
        ref = per_step_counts.clone()
        if world > 1:
            ref = allreduce(per_step_counts.to(dev), _sum(), world).cpu()
        legs["montecarlo"] = mc_leg(code, snrs, B, cw0, world, timer, dev, ref)
    if not args.no_gru:
        legs["headline_kernel_decoding_net"] = decoding_net_leg(dev, rank, world, timer)
        legs["crisp_gru"] = gru_leg(code, dev, ys[2], B, world, timer)
        legs["crisp_gru_f512"] = crisp_f512_leg(dev, rank, world, timer)
    if not (args.no_gru and args.no_pac):
        legs.update(pac_legs(snrs, B, rank, world, timer, dev, not args.no_gru, not args.no_pac))
    if not args.no_gru:
        legs["pac_gru_decoding_net"] = decoding_net_leg(dev, rank, world, timer, path=TRAINED_PAC_32_10)
    if not args.no_scl:
        legs["scl"] = scl_leg(code, dev, ys[2], snrs[2], world, timer)
    if not args.no_lse:
        legs["sc_lse"] = lse_leg(code, dev, ys[2], snrs[2], world, timer)
    if not args.no_conv:
        legs["conv_model"] = conv_leg(dev, rank, world, timer)

    if rank != 0:
        return 0
    if not args.no_traffic and world == 1:
        traffic, how, raw = pmc_traffic(args)
        if traffic is not None:
            headline["roofline"]["traffic"] = traffic[GRU_KERNEL]
            headline["roofline"]["traffic_raw"] = raw[GRU_KERNEL]
            headline["roofline"]["sc_launch"]["traffic"] = traffic[KERNEL_NAME.split("<")[0]]
            sc1["roofline"]["traffic"] = traffic[KERNEL_NAME.split("<")[0]]
            if "pac_sc" in legs:
                legs["pac_sc"]["roofline"]["traffic"] = traffic[PAC_KERNEL]
        headline["roofline"]["traffic_source"] = how
    if not args.no_cpu_baseline and world == 1:
        net32, _, _, _ = crisp_model(code, dev)
        yh = [y[:4096].cpu().numpy() for y in ys]
        headline["cpu_baseline"] = cpu_baseline_sc_gru(yh, snrs, info, net32, args.cpu_seconds)
        ys_host = [y[: 1 << 18].cpu().numpy() for y in ys]
        sc1["cpu_baseline"] = cpu_baseline(ys_host, snrs, info, args.cpu_seconds)
    full.update(legs)
    try:
        os.makedirs(os.path.dirname(os.path.abspath(args.full_json)), exist_ok=True)
        with open(args.full_json, "w") as f:
            json.dump(full, f, indent=1)
        headline["full_record"] = os.path.relpath(os.path.abspath(args.full_json), ROOT)
    except OSError as e:
        headline["full_record"] = f"not written: {e}"
    headline.update(compact_configs(legs, gvr))
    print(json.dumps(_round_floats(headline)), flush=True)
    return 0


def _round_floats(x, keep=("value", "ms_per_step")):
    """5 significant digits for the printed line (the full record keeps full precision)."""
    if isinstance(x, dict):
        return {k: (v if k in keep else _round_floats(v, keep)) for k, v in x.items()}
    if isinstance(x, list):
        return [_round_floats(v, keep) for v in x]
    if isinstance(x, float):
        return float(f"{x:.5g}")
    return x


def compact_configs(legs, gvr):
    """One small summary per configuration for the printed line (the full records are in the --full-json file)."""
    def r3(x):
        return None if x is None else float(f"{x:.4g}")

    out = {"gru_vs_reference_within_4_sigma": None if gvr is None else gvr["within_4_sigma"]}
    dn = legs.get("headline_kernel_decoding_net")
    if dn is not None:
        # the headline kernel's BER match, measured on a net that decodes (the headline net's BLER is ~1)
        out["headline_kernel_ber_match"] = {
            "net": "trained_crisp_32_16 (Polar(32,16), hidden 64; reference BLER 0.73 -> 0.16 over 0-4 dB)",
            "within_4_sigma": dn["gru_vs_reference"]["within_4_sigma"],
            "ber_match_0.05dB": dn["db_bar"]["ber_match_0.05dB"],
            "resolvable_points": dn["db_bar"]["resolvable_points"],
            "bler_db_offset": {k: r3(v["offset_db"]) for k, v in dn["db_bar"]["points"].items()}}
    c = {}
    if "configs1_sc" in legs:
        l1 = legs["configs1_sc"]
        c["1_sc_decode"] = {"value": r3(l1["value"]), "hbm_frac": r3(l1["roofline"]["frac"]),
                            "ber_match_0.05dB": l1.get("ber_match")}
    if "fp32_path" in legs:
        c["1+2_step_fp32_gru"] = {"value": r3(legs["fp32_path"]["value"]),
                                  "fp32_mfma_frac": r3(legs["fp32_path"]["roofline"]["frac"])}
    if "crisp_gru" in legs:
        g = legs["crisp_gru"]
        c["2_crisp_gru_alone"] = {"fp32": r3(g["value"]), "fp16x3_launch_ms": r3(g["fp16x3"]["avg_launch_ms"])}
    if "pac_gru" in legs:
        c["3_pac_gru"] = {"value": r3(legs["pac_gru"]["value"]), "fp16_issued_frac": r3(legs["pac_gru"]["issued_frac"]),
                          "fp32_path": r3(legs["pac_gru"]["fp32_path"]["value"])}
    pn = legs.get("pac_gru_decoding_net")
    if pn is not None and "3_pac_gru" in c:
        # configs[3]'s kernel on a PAC net that decodes (scaled down: PAC(32,10), g = 53, hidden 64)
        c["3_pac_gru"]["trained_scaled_down_ber_match_0.05dB"] = pn["db_bar"]["ber_match_0.05dB"]
        c["3_pac_gru"]["trained_scaled_down_within_4_sigma"] = pn["gru_vs_reference"]["within_4_sigma"]
    if "pac_sc" in legs:
        c["3_pac_sc"] = {"value": r3(legs["pac_sc"]["value"]), "hbm_frac": r3(legs["pac_sc"]["roofline"]["frac"])}
    if "conv_model" in legs:
        cm = legs["conv_model"]
        c["4_conv_model"] = {"value": r3(cm["value"]), "fp16_issued_frac": r3(cm["roofline"]["frac"]),
                             "fp32_path": r3(cm["fp32_path"]["value"])}
        for k in ("trained_scaled_down", "trained_run_alt_e128"):
            if cm.get(k):
                c["4_conv_model"][k + "_ber_match_0.05dB"] = cm[k]["db_bar"]["ber_match_0.05dB"]
    if "montecarlo" in legs:
        c["montecarlo_fused_sc"] = r3(legs["montecarlo"]["value"])
    if "crisp_gru_f512" in legs:
        f = legs["crisp_gru_f512"]
        c["crisp_f512"] = {"value": r3(f["value"]), "fp32_mfma_frac": r3(f["frac"]),
                           "within_4_sigma": (f.get("gru_vs_reference") or {}).get("within_4_sigma")}
    out["configs_summary"] = c
    return out


if __name__ == "__main__":
    sys.exit(main())
