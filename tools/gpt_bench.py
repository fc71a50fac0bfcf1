"""GPT transformer decode throughput on cuda:0: the fused kernel against a torch restatement on the same card.

    python tools/gpt_bench.py [--out FILE.json] [--quick] [--layers 6]

Configurations: Polar(32,16) and Polar(64,32), 6 layers, embed_dim 64, 8 heads, B = 4096 words at 2 dB; seeded weights
(2-D parameters x 3, as the test fixtures).  Per configuration, after two warm-up calls, SAMPLES timed windows (device
events around enough back-to-back calls to last >= 0.1 s each); the median window gives the time per call.  Reported:
  * codewords/s of npd_gpt_decode (bits and logits);
  * FLOP/s by the decode's own count, layers x sum over information positions of (12 E^2 n + 2 E n^2) MACs with
    n = i + 1, as a fraction of the fp32 MFMA peak (157 TFLOP/s, the card's spec figure);
  * the torch baseline: the same prefix-only decode (tokens 0 .. i only, every key <= i visible) in fp32 torch ops on
    the same card, batched over the B words -- what a user gets by restating the reference's decode without its dead
    work; its logits are compared with the kernel's along the kernel's own decided path.
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
import neural_polar_decoder_amd as npd  # noqa: E402
from neural_polar_decoder_amd.montecarlo import seeded_gpt  # noqa: E402

PEAK_FP32_MFMA = 157e12
SAMPLES = 5
SNR = 2.0
E = 64


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


def macs_per_word(info, layers):
    return layers * sum(12 * E * E * (i + 1) + 2 * E * (i + 1) ** 2 for i in info)


@torch.no_grad()
def torch_prefix_decode(net, y, info, forced=None):
    """The prefix-only decode in fp32 torch ops: (bits, logits), both (B, N)."""
    B, N = y.shape
    H, d = net.n_head, net.embed_dim // net.n_head
    start = net.start_embed_layer(y)
    pos_emb = net.pos_emb.weight
    table = net.Decoder.position_enc_auto.pos_table[0]
    feed = torch.ones(B, N, device=y.device) if forced is None else forced.clone()
    bits, logits = torch.ones(B, N, device=y.device), torch.zeros(B, N, device=y.device)
    for i in info:
        n = i + 1
        x = torch.cat((start.unsqueeze(1), feed[:, :i, None] * pos_emb[None, 1:n]), 1) + table[None, :n]
        for layer in net.Decoder.layer_stack:
            at, ff = layer.slf_attn, layer.pos_ffn
            q = at.w_qs(x).view(B, n, H, d).transpose(1, 2)
            k = at.w_ks(x).view(B, n, H, d).transpose(1, 2)
            v = at.w_vs(x).view(B, n, H, d).transpose(1, 2)
            a = torch.softmax(torch.matmul(q / at.attention.temperature, k.transpose(2, 3)), -1)
            o = torch.matmul(a, v).transpose(1, 2).reshape(B, n, H * d)
            x = at.layer_norm(at.fc(o) + x)
            x = ff.layer_norm(ff.w_2(F.gelu(ff.w_1(x))) + x)
        lg = net.Lin_Decoder(x[:, i])[:, 0]
        logits[:, i] = lg
        bits[:, i] = lg.sign()
        if forced is None:
            feed[:, i] = bits[:, i]
    return bits, logits


def bench(N, K, layers, B):
    dev = torch.device("cuda:0")
    code = npd.reference_polar_code(N, K)
    info = [int(i) for i in code.info_positions]
    net = seeded_gpt(N, layers, seed=11, device=dev)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 2:
                p.mul_(3.0)
    _, _, y = code.mc_generate(B, SNR, seed=1, device=dev, want_msg=False)
    rec = {"code": f"polar({N},{K})", "layers": layers, "B": B, "snr_db": SNR}
    t, lo, hi, reps = time_call(lambda: net.decode_logits(y, info))
    flops = 2.0 * macs_per_word(info, layers) * B
    rec["kernel"] = {"s_per_call": t, "min": lo, "max": hi, "calls_per_window": reps, "cw_per_s": B / t,
                     "flops": flops / t, "frac_fp32_mfma_peak": flops / t / PEAK_FP32_MFMA}
    t, lo, hi, reps = time_call(lambda: torch_prefix_decode(net, y, info))
    rec["torch_fp32_prefix_decode"] = {"s_per_call": t, "min": lo, "max": hi, "calls_per_window": reps, "cw_per_s": B / t}
    bits, lg = net.decode_logits(y, info)
    _, tl = torch_prefix_decode(net, y, info, forced=bits)
    rec["max_abs_logit_diff_on_kernel_path"] = float((tl - lg)[:, info].abs().max())
    rec["speedup_over_torch"] = rec["kernel"]["cw_per_s"] / rec["torch_fp32_prefix_decode"]["cw_per_s"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--quick", action="store_true", help="1/16 of the batch (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpt_bench needs the GPU: there is no CPU path to time")
    out = []
    for N, K in [(32, 16), (64, 32)]:
        rec = bench(N, K, a.layers, 4096 // (16 if a.quick else 1))
        out.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
