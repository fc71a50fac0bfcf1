"""Train a CRISP GRU on the fused training kernels: the reference's loop (rnn_all.py:1386-1440) over this package's
classes, with the reference's flag names.

    python -m neural_polar_decoder_amd.train --N 16 --K 4 --rnn_feature_size 32 --rnn_depth 1 --num_steps 100 \
        --save_path crisp.pt

Per step: msg / y from the code's mc_generate (Philox, on the GPU), the teacher forcing ratio of the reference's decay,
RNN_decoder.decode(net, True, y, gt, tfr) (one fused forward launch), the loss on the information positions,
(loss / mult).backward() (the fused backward recurrence and the weight-gradient contraction), clip_grad_norm_, and an
AdamW step every `mult` steps.  The checkpoint is the reference's {'net', 'step', 'args'}, which
datasets.rnn_from_checkpoint loads.
"""
from __future__ import annotations

import argparse
import math

import numpy as np
import torch
import torch.nn as nn


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    # code
    p.add_argument("--code", default="Polar", choices=["Polar", "PAC", "polar", "pac"])
    p.add_argument("--N", type=int, default=16)
    p.add_argument("--K", type=int, default=8)
    p.add_argument("--target_K", type=int, default=None)
    p.add_argument("--rate_profile", default="polar")
    p.add_argument("--g", type=int, default=None, help="PAC convolution polynomial (octal digits read as decimal, e.g. 91)")
    # net
    p.add_argument("--rnn_feature_size", type=int, default=64)
    p.add_argument("--rnn_depth", type=int, default=2)
    p.add_argument("--onehot", action="store_true")
    p.add_argument("--reverse_order", action="store_true")
    # run
    p.add_argument("--num_steps", type=int, default=1000)
    p.add_argument("--batch_size", type=int, default=4096)
    p.add_argument("--dec_train_snr", type=float, default=0.0)
    p.add_argument("--load_path", default=None)
    p.add_argument("--save_path", default=None)
    p.add_argument("--random_seed", type=int, default=42)
    p.add_argument("--print_freq", type=int, default=100)
    p.add_argument("--gpu", type=int, default=0)
    # teacher forcing
    p.add_argument("--tfr_min", type=float, default=0.0)
    p.add_argument("--tfr_max", type=float, default=0.0)
    p.add_argument("--tfr_decay", type=float, default=10000.0)
    p.add_argument("--teacher_steps", type=int, default=-10000)
    # loss and optimiser
    p.add_argument("--loss", default="MSE", choices=["MSE", "BCE"])
    p.add_argument("--clip", type=float, default=1.0)
    p.add_argument("--mult", type=int, default=1)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--scheduler", default=None, choices=[None, "step"])
    p.add_argument("--lr_decay", type=int, default=1000)
    p.add_argument("--lr_decay_gamma", type=float, default=0.9)
    a = p.parse_args(argv)
    if a.target_K is None:
        a.target_K = a.K
    if a.g is None:
        delattr(a, "g")  # code_from_args then takes the reference's default polynomial for this N
    # what rnn_from_checkpoint reads to rebuild the net (the CRISP scripts' configuration)
    a.rnn_type, a.decoding_type, a.use_ynn, a.out_linear_depth, a.dropout = "GRU", "y_input", False, 1, 0.0
    a.bidirectional, a.use_layernorm = False, False
    return a


def tfr_of(args, i_step):
    """rnn_all.py:1399."""
    if i_step > args.teacher_steps:
        return args.tfr_min + (args.tfr_max - args.tfr_min) * math.exp(-1 * (i_step - args.teacher_steps) / args.tfr_decay)
    return args.tfr_max


def train(args, device=None, log=print):
    """Run the loop; returns (net, decoder, code, losses)."""
    from .datasets import code_from_args, load_checkpoint
    from .rnn import RNN_Model, RNN_decoder
    device = torch.device(device if device is not None else f"cuda:{args.gpu}")
    torch.manual_seed(args.random_seed)
    code = code_from_args(args)
    info = getattr(code, "info_positions", None)
    info = np.asarray(info if info is not None else code.B, np.int64)  # message column k sits at position info[k]
    info_t = torch.as_tensor(info, device=device)
    net = RNN_Model("GRU", args.N + 1 + int(args.onehot), args.rnn_feature_size, 1, args.rnn_depth, args.N, 0, 0, "selu",
                    0.0, False, out_linear_depth=1).to(device)
    if args.load_path:
        net.load_state_dict(load_checkpoint(args.load_path)["net"])
    decoder = RNN_decoder("y_input", args.N, info.tolist(), onehot=args.onehot, reverse_order=args.reverse_order)
    why = decoder.train_reason(net)
    if why is not None:
        from ._lib import NpdError
        raise NpdError(why)
    optimizer = torch.optim.AdamW(net.parameters(), lr=args.lr)
    scheduler = (torch.optim.lr_scheduler.StepLR(optimizer, args.lr_decay, args.lr_decay_gamma)
                 if args.scheduler == "step" else None)
    loss_fn = nn.MSELoss() if args.loss == "MSE" else nn.BCEWithLogitsLoss()
    losses = []
    optimizer.zero_grad()
    for i_step in range(args.num_steps):
        msg, _, y = code.mc_generate(args.batch_size, args.dec_train_snr, seed=args.random_seed, snr_index=0,
                                     cw_offset=i_step * args.batch_size, device=device)
        gt = torch.ones(args.batch_size, args.N, device=device)
        gt[:, info_t] = msg
        decoded = decoder.decode(net, True, y, gt, tfr_of(args, i_step))
        dmsg = decoded[:, info_t]
        loss = loss_fn(dmsg, 0.5 + 0.5 * msg) if args.loss == "BCE" else loss_fn(dmsg, msg)
        (loss / args.mult).backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), args.clip)
        if i_step % args.mult == 0:
            optimizer.step()
            optimizer.zero_grad()
            if scheduler is not None:
                scheduler.step()
        losses.append(loss.detach())
        if args.print_freq and i_step % args.print_freq == 0:
            ber = float((dmsg.detach().sign() != msg).float().mean())
            log(f"[{i_step}/{args.num_steps}] loss {float(losses[-1]):.6f} train BER {ber:.5f}")
    losses = [float(x) for x in torch.stack(losses).cpu()] if losses else []
    if args.save_path:
        torch.save({"net": {k: v.detach().cpu() for k, v in net.state_dict().items()}, "step": args.num_steps,
                    "args": args}, args.save_path)
    return net, decoder, code, losses


def main(argv=None):
    args = parse_args(argv)
    _, _, _, losses = train(args)
    if losses:
        print(f"done: {len(losses)} steps, first loss {losses[0]:.6f}, last loss {losses[-1]:.6f}")


if __name__ == "__main__":
    main()
