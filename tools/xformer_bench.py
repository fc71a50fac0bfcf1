"""Encoder / decoder transformer model throughput on cuda:0: the fused kernels against torch restatements on the same
card, and the decoder beside the GPT decode.

    python tools/xformer_bench.py [--out FILE.json] [--quick] [--layers 6]

Configurations: Polar(32,16) and Polar(64,32), 6 layers, embed_dim 64, 8 heads, B = 4096 words at 2 dB; seeded weights
(2-D parameters x 3, as the test fixtures).  Per configuration, after two warm-up calls, SAMPLES timed windows (device
events around enough back-to-back calls to last >= 0.1 s each); the median window gives the time per call.  Reported:
  * codewords/s of npd_xfdec_decode and npd_xfenc_forward (bits and logits), and of npd_gpt_decode at the same
    (N, layers) in the same run;
  * FLOP/s by each function's own MAC count as a fraction of the fp32 MFMA peak (157 TFLOP/s, the card's spec figure).
    Decoder, per word: layers x (2 E^2 N for the memory's keys and values, once, + the sum over information positions
    of 14 E^2 n + 2 E n^2 + 2 E n N, n = i + 1).  The kernel recomputes the memory's keys and values at every step;
    that work is not counted as useful, and its share of the MACs the kernel executes is reported.  Encoder, per word:
    layers x (12 E^2 N + 2 E N^2);
  * the torch baselines, fp32 on the same card, batched over the B words, each in its most favourable form: for the
    decoder the prefix-only decode (tokens 0 .. i only, every key <= i visible) with the memory's keys and values
    computed once per layer; for the encoder one batched forward without a mask.  Their logits are compared with the
    kernel's (the decoder's along the kernel's own decided path).
"""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import neural_polar_decoder_amd as npd  # noqa: E402
from neural_polar_decoder_amd.montecarlo import seeded_gpt, seeded_xformer  # noqa: E402
from gpt_bench import PEAK_FP32_MFMA, SNR, E, time_call  # noqa: E402


def dec_macs_per_word(info, layers, N, recompute=False):
    steps = sum(14 * E * E * (i + 1) + 2 * E * (i + 1) ** 2 + 2 * E * (i + 1) * N for i in info)
    return layers * (steps + 2 * E * E * N * (len(info) if recompute else 1))


def enc_macs_per_word(layers, N):
    return layers * (12 * E * E * N + 2 * E * N * N)


def _attend(at, xq, xk, xv_heads=None):
    B, n, H = xq.shape[0], xq.shape[1], at.n_head
    d = xq.shape[2] // H
    q = at.w_qs(xq).view(B, n, H, d).transpose(1, 2)
    k, v = xv_heads if xv_heads is not None else _kv(at, xk)
    a = torch.softmax(torch.matmul(q / at.attention.temperature, k.transpose(2, 3)), -1)
    o = torch.matmul(a, v).transpose(1, 2).reshape(B, n, H * d)
    return at.layer_norm(at.fc(o) + xq)


def _kv(at, x):
    B, n, H = x.shape[0], x.shape[1], at.n_head
    d = x.shape[2] // H
    return at.w_ks(x).view(B, n, H, d).transpose(1, 2), at.w_vs(x).view(B, n, H, d).transpose(1, 2)


@torch.no_grad()
def torch_prefix_decode(net, y, info, forced=None):
    """The decoder's prefix-only decode in fp32 torch ops, the memory's keys and values once per layer: (bits, logits)."""
    B, N = y.shape
    dec = net.Decoder
    mem = dec.layer_norm_cross(y.unsqueeze(-1) * dec.emb_cross.weight[None, 1:N + 1] + dec.position_enc_cross.pos_table[:, :N])
    cross = [_kv(layer.enc_attn, mem) for layer in dec.layer_stack]
    tokens = dec.layer_norm(dec.emb_inputs.weight[:3, None, :] + dec.position_enc_auto.pos_table[:, :N])  # (3, N, E)
    feed = torch.ones(B, N, device=y.device) if forced is None else forced.clone()
    bits, logits = torch.ones(B, N, device=y.device), torch.zeros(B, N, device=y.device)
    pos = torch.arange(N, device=y.device)
    for i in info:
        n = i + 1
        idx = torch.cat((torch.full((B, 1), 2, dtype=torch.long, device=y.device), (feed[:, :i] == 1).long()), 1)
        x = tokens[idx, pos[None, :n]]
        for layer, kv in zip(dec.layer_stack, cross):
            x = _attend(layer.slf_attn, x, x)
            x = _attend(layer.enc_attn, x, None, kv)
            ff = layer.pos_ffn
            x = ff.layer_norm(ff.w_2(F.gelu(ff.w_1(x))) + x)
        lg = net.Lin_Decoder(x[:, i])[:, 0]
        logits[:, i] = lg
        bits[:, i] = lg.sign()
        if forced is None:
            feed[:, i] = bits[:, i]
    return bits, logits


@torch.no_grad()
def torch_encoder_forward(net, y):
    return net(y, None, None, y.device)[3][:, :, 0]


def _timed(fn, B, flops=None):
    t, lo, hi, reps = time_call(fn)
    r = {"s_per_call": t, "min": lo, "max": hi, "calls_per_window": reps, "cw_per_s": B / t}
    if flops is not None:
        r.update(flops=flops / t, frac_fp32_mfma_peak=flops / t / PEAK_FP32_MFMA)
    return r


def bench(N, K, layers, B):
    dev = torch.device("cuda:0")
    code = npd.reference_polar_code(N, K)
    info = [int(i) for i in code.info_positions]
    nets = {"decoder": seeded_xformer("decoder", N, layers, seed=11, device=dev),
            "encoder": seeded_xformer("encoder", N, layers, seed=11, device=dev), "gpt": seeded_gpt(N, layers, seed=11, device=dev)}
    with torch.no_grad():
        for net in nets.values():
            for p in net.parameters():
                if p.dim() == 2:
                    p.mul_(3.0)
    _, _, y = code.mc_generate(B, SNR, seed=1, device=dev, want_msg=False)
    rec = {"code": f"polar({N},{K})", "layers": layers, "B": B, "snr_db": SNR}
    dec, enc, gpt = nets["decoder"], nets["encoder"], nets["gpt"]
    useful, executed = dec_macs_per_word(info, layers, N), dec_macs_per_word(info, layers, N, recompute=True)
    d = rec["decoder"] = {"kernel": _timed(lambda: dec.decode_logits(y, info), B, 2.0 * useful * B),
                          "macs_per_word": useful, "macs_per_word_executed": executed,
                          "recompute_share_of_executed_macs": (executed - useful) / executed,
                          "torch_fp32_prefix_decode": _timed(lambda: torch_prefix_decode(dec, y, info), B),
                          "gpt_kernel_same_shape": _timed(lambda: gpt.decode_logits(y, info), B)}
    bits, lg = dec.decode_logits(y, info)
    _, tl = torch_prefix_decode(dec, y, info, forced=bits)
    d["max_abs_logit_diff_on_kernel_path"] = float((tl - lg)[:, info].abs().max())
    d["speedup_over_torch"] = d["kernel"]["cw_per_s"] / d["torch_fp32_prefix_decode"]["cw_per_s"]
    d["cw_per_s_relative_to_gpt"] = d["kernel"]["cw_per_s"] / d["gpt_kernel_same_shape"]["cw_per_s"]
    e = rec["encoder"] = {"kernel": _timed(lambda: enc.logits(y), B, 2.0 * enc_macs_per_word(layers, N) * B),
                          "macs_per_word": enc_macs_per_word(layers, N),
                          "torch_fp32_forward": _timed(lambda: torch_encoder_forward(enc, y), B)}
    e["max_abs_logit_diff"] = float((torch_encoder_forward(enc, y) - enc.logits(y)[0]).abs().max())
    e["speedup_over_torch"] = e["kernel"]["cw_per_s"] / e["torch_fp32_forward"]["cw_per_s"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--quick", action="store_true", help="1/16 of the batch (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xformer_bench needs the GPU: there is no CPU path to time")
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
