"""Train the convNet decoder on the fused training kernels: the reference's loop (run_models.py:826-915) for
``--model conv --loss MSE`` over this package's convNet, with the reference's flag names.

    python -m neural_polar_decoder_amd.train_conv --N 64 --K 1 --target_K 22 --embed_dim 128 --batch_size 8192 \
        --dec_train_snr -6 --num_steps 1000 --save_path stage1.pt
    python -m neural_polar_decoder_amd.train_conv --N 64 --K 2 --target_K 22 ... --load_previous --load_path stage1.pt

Per step (run_models.py:840-915): msg = 1 - 2 (rand < 0.5) (B, K); gt = ones (B, N), gt[:, info] = msg; y =
encode_plotkin(msg at info) + sigma(dec_train_snr) randn; convNet.forward in training mode (one fused forward; dropout
drawn in Python); loss = MSE(logits[:, info], gt[:, info]) (out_mask is all ones); (loss / mult).backward() (the fused
backward); clip_grad_norm_(clip); an AdamW step every `mult` steps.  A stage is one invocation, as in run_alt.sh /
run_conv_c2n.sh: --load_previous starts it from the previous stage's checkpoint and a fresh optimiser, and the caller
passes the stage's --dec_train_snr (the scripts' ramp).

Information sets (run_models.py:658-669, as tests/golden/train_conv_gpu.py derives them): rs = the reliability sequence
below N; n2c: sort(flip(rs[:target_K])[:K]), the K least reliable positions of the target's set; c2n: sort(rs[:K]).

The checkpoint is the reference's {'xformer', 'step', 'args'}, which datasets.convnet_from_checkpoint loads.
"""
from __future__ import annotations

import argparse

import numpy as np
import torch
import torch.nn as nn


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--N", type=int, default=64)
    p.add_argument("--K", type=int, default=22)
    p.add_argument("--target_K", type=int, default=None)
    p.add_argument("--curriculum", default="n2c", choices=["n2c", "c2n"])
    p.add_argument("--embed_dim", type=int, default=128)
    p.add_argument("--dropout", type=float, default=0.1)
    p.add_argument("--dont_use_bias", action="store_true")
    p.add_argument("--num_steps", type=int, default=1000)
    p.add_argument("--batch_size", type=int, default=8192)
    p.add_argument("--dec_train_snr", type=float, default=0.0)
    p.add_argument("--loss", default="MSE", choices=["MSE"])
    p.add_argument("--clip", type=float, default=0.25)
    p.add_argument("--mult", type=int, default=1)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--optimizer_type", default="AdamW", choices=["AdamW"])
    p.add_argument("--load_previous", action="store_true", help="start from --load_path's weights (the previous stage)")
    p.add_argument("--load_path", default=None)
    p.add_argument("--save_path", default=None)
    p.add_argument("--random_seed", type=int, default=42)
    p.add_argument("--print_freq", type=int, default=100)
    p.add_argument("--gpu", type=int, default=0)
    a = p.parse_args(argv)
    if a.target_K is None:
        a.target_K = a.K
    if not 1 <= a.K <= a.target_K <= a.N:
        p.error("need 1 <= K <= target_K <= N")
    if a.load_previous and not a.load_path:
        p.error("--load_previous needs --load_path")
    # what convnet_from_checkpoint and the reference's convNet(args) read
    a.model, a.code, a.rate_profile, a.max_len = "conv", "polar", "polar", a.N
    return a


def stage_info(N, target_K, K, curriculum="n2c"):
    """The stage's sorted information positions."""
    from .codes import polar_rs
    rs = polar_rs(N)
    if curriculum == "c2n":
        return np.sort(rs[:K]).astype(np.int64)
    return np.sort(np.flip(rs[:target_K])[:K].copy()).astype(np.int64)


def plotkin(u):
    """x = u F^{(x)n} in BPSK (polar.py:128-148 encode_plotkin on the full-length u)."""
    B, N = u.shape
    x = u.clone()
    s = 1
    while s < N:
        v = x.view(B, N // (2 * s), 2, s)
        v[:, :, 0, :] = v[:, :, 0, :] * v[:, :, 1, :]
        s *= 2
    return x


def train(args, device=None, log=print):
    """Run one stage; returns (net, info positions, losses)."""
    from ._lib import NpdError
    from .datasets import load_checkpoint
    from .models import convNet
    from .utils import snr_db2sigma
    device = torch.device(device if device is not None else f"cuda:{args.gpu}")
    torch.manual_seed(args.random_seed)
    info = stage_info(args.N, args.target_K, args.K, args.curriculum)
    info_t = torch.as_tensor(info, device=device)
    net = convNet(args)
    loaded = 0
    if args.load_previous:
        ck = load_checkpoint(args.load_path)
        net.load_state_dict(ck["xformer"])
        loaded = int(ck.get("step", 0))
        log(f"Training Model for {args.K},{args.N} loaded at step {loaded} from {args.load_path}")
    net.to(device).train()
    why = net.train_reason()
    if why is not None:
        raise NpdError(why)
    optimizer = torch.optim.AdamW(net.parameters(), lr=args.lr)
    loss_fn = nn.MSELoss()
    sigma = snr_db2sigma(args.dec_train_snr)
    mask = torch.ones(args.batch_size, args.N, device=device).long()
    losses = []
    optimizer.zero_grad()
    for i_step in range(args.num_steps):
        msg = 1 - 2 * (torch.rand(args.batch_size, args.K, device=device) < 0.5).float()
        gt = torch.ones(args.batch_size, args.N, device=device)
        gt[:, info_t] = msg
        y = plotkin(gt) + sigma * torch.randn(args.batch_size, args.N, device=device)
        _, decoded, out_mask, logits, _ = net(y, mask, gt, device)
        loss = loss_fn(out_mask[:, info_t] * logits[:, info_t, 0], out_mask[:, info_t] * gt[:, info_t])
        (loss / args.mult).backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), args.clip)
        if i_step % args.mult == 0:
            optimizer.step()
            optimizer.zero_grad()
        losses.append(loss.detach())
        if args.print_freq and i_step % args.print_freq == 0:
            ber = float((decoded[:, info_t, 0] != msg).float().mean())
            log(f"[{i_step}/{args.num_steps}] loss {float(losses[-1]):.6f} train BER ({args.dec_train_snr:g} dB) {ber:.5f}")
    losses = [float(x) for x in torch.stack(losses).cpu()] if losses else []
    if args.save_path:
        torch.save({"xformer": {k: v.detach().cpu() for k, v in net.state_dict().items()}, "step": args.num_steps,
                    "args": args}, args.save_path)
    return net, info, losses


def main(argv=None):
    args = parse_args(argv)
    _, _, losses = train(args)
    if losses:
        k = max(1, len(losses) // 10)
        print(f"done: {len(losses)} steps, mean loss of the first {k} steps {np.mean(losses[:k]):.6f}, of the last {k} "
              f"{np.mean(losses[-k:]):.6f}")


if __name__ == "__main__":
    main()
