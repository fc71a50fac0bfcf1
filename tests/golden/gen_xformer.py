#!/usr/bin/env python3
"""Encoder / decoder transformer fixtures: tests/golden/xfenc_polar_*.npz and xfdec_polar_*.npz, from the reference's
XFormerEndToEndEncoder (models.py:662-686) and XFormerEndToEndDecoder (models.py:599-654).

Run in the build container only (``/root/reference`` does not exist on the GPU box; without it the script says so and
writes nothing):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_xformer.py

models.py imports IPython, which is not installed: a stub module stands in for it.

The masking switch.  The reference's ScaledDotProductAttention branches on a module-level ``MODEL = 'gpt'``; the
``MODEL = config.model`` lines in the constructors are local assignments and change nothing.  With the file as shipped
both classes raise a shape error at every batch size other than 1 or 8 (the mask lines up with the head axis).  This
script sets ``models.MODEL = config.model`` before it builds a class: the non-'gpt' branch is the only reading under
which the classes run at a general batch size.

Weights.  torch.manual_seed(11), the reference's class with PyTorch's default initialisation, then every 2-D parameter
x 3: at the default scale the decoder's decisions ignore y.  A fixture that would pass the size limit of a committed
file with its state dict inside stores the seed and a sha256 of the state dict instead, and tests/xformer_helper.py
regenerates the weights with this package's class (same draws, same order -- checked here against the reference's for
every fixture).

Words.  Polar(N, K) codewords at 2 dB; for the decoder a second set with random +-1 forced paths of N bits.

Stored per fixture: the state-dict key list; y, the reference's decode() bits and the fp32 logits behind them (decoder:
its own modules stepped as decode steps them and checked to give decode()'s bits; encoder: forward()'s); decoder:
y_forced, forced and the fp32 logits along the forced paths; e_ref = max |reference fp32 - float64 restatement| over the
compared logits (decoder: information logits of the forced paths; encoder: all N logits of y); the reference's
forward() logits on 4 words (decoder: (4 N, N), trg_seq = the forced paths).

Asserted here, so that no test can hide behind them: at least 0.9 of the words are robust (min |float64 logit| >= 10 tol,
over the information positions for the decoder, over all N for the encoder) and the reference's bits equal the float64
bits on every robust word.  If a seed misses either, change the seed.
"""
import argparse
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(OUT)
ROOT = os.path.dirname(TESTS)

import numpy as np  # noqa: E402
import torch  # noqa: E402

W_SEED = 11
SIZE_LIMIT = 488076  # bytes: the largest transformer fixture committed before these
SHAPES = [dict(tag="16_8_l1", N=16, K=8, L=1, n=96, seed_y=201),
          dict(tag="32_16_l2", N=32, K=16, L=2, n=96, seed_y=202),
          dict(tag="64_32_l2", N=64, K=32, L=2, n=48, seed_y=203),
          dict(tag="32_16_l6", N=32, K=16, L=6, n=96, seed_y=204),
          dict(tag="64_32_l6", N=64, K=32, L=6, n=32, seed_y=205)]
STORE_WEIGHTS_UP_TO = dict(decoder=1, encoder=2)  # layers
FWD_WORDS = 4


def words(N, K, info, n, seed, O):
    torch.manual_seed(seed)
    msg = 1.0 - 2.0 * (torch.rand(n, K) < 0.5).float()
    x = torch.from_numpy(O.encode_plotkin(msg.numpy(), N, info))
    sigma = 10 ** (-2.0 / 20)
    return (x + sigma * torch.randn(x.shape)).numpy().astype(np.float32)


def stepped_dec(net, y, info, forced=None):
    """The reference's modules stepped as its decode steps them (models.py:635-654), keeping the logits."""
    dev = torch.device("cpu")
    B, N = y.shape
    with torch.no_grad():
        mask = torch.ones(B, N).bool()
        enc_input = torch.ones(net.embed_dim) * y.unsqueeze(-1)
        seq = torch.ones((B, N)).long()
        seq[:, 0] = 2
        tri = torch.tril(torch.ones((1, N, N))).bool() & mask.unsqueeze(1)
        bits, logits = torch.ones((B, N)), torch.zeros((B, N))
        for i in range(N):
            nb = torch.ones(B)
            if i in info:
                lg = net.Lin_Decoder(net.Decoder(enc_input, mask, seq, tri[:, i, :], dev))[:, i, 0]
                logits[:, i] = lg
                nb = lg.sign()
            bits[:, i] = nb
            if i < N - 1:
                feed = nb if forced is None else forced[:, i]
                seq[:, i + 1] = (feed == 1).long()
    return bits.numpy(), logits.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    if not os.path.isdir(REF):
        print(f"gen_xformer: {REF} is absent -- nothing generated")
        return 0
    for p in (ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    import xformer_helper as X
    from conftest import weights_digest
    from neural_polar_decoder_amd.codes import polar_info_positions
    from oracle import oracle as O
    stub = types.ModuleType("IPython")
    stub.display = None
    stub.version_info = (8, 30, 0)
    stub.get_ipython = lambda: None
    sys.modules.setdefault("IPython", stub)
    sys.path.insert(0, REF)
    import models as R  # the reference's
    torch.set_num_threads(8)
    dev = torch.device("cpu")
    for model in X.MODELS:
        for c in SHAPES:
            name = ("xfdec" if model == "decoder" else "xfenc") + "_polar_" + c["tag"]
            if a.only and a.only != name:
                continue
            N, K, L, n = c["N"], c["K"], c["L"], c["n"]
            info = np.sort(np.asarray(polar_info_positions(N, K, "polar", None))).astype(np.int64)
            is_info = np.zeros(N, np.uint8)
            is_info[info] = 1
            cfg = X.xf_config(model, N, L)
            R.MODEL = cfg.model  # the non-'gpt' masking branch (see the module docstring)
            torch.manual_seed(W_SEED)
            net = (R.XFormerEndToEndDecoder if model == "decoder" else R.XFormerEndToEndEncoder)(cfg).eval()
            with torch.no_grad():
                for p in net.parameters():
                    if p.dim() == 2:
                        p.mul_(X.INIT_SCALE)
            sd = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
            ours = X.seeded_state_dict(model, N, L, W_SEED)
            assert list(ours) == list(sd) and weights_digest(ours) == weights_digest(sd), "this package's class draws differently"
            y = words(N, K, info, n, c["seed_y"], O)
            yt = torch.from_numpy(y)
            ones = torch.ones(n, N).bool()
            out = dict(N=N, K=K, n_layers=L, info=info, is_info=is_info, keys=np.array(list(sd)), y=y,
                       w_scale=X.INIT_SCALE)
            if model == "decoder":
                yf = words(N, K, info, n, c["seed_y"] + 1000, O)
                torch.manual_seed(c["seed_y"] + 2000)
                forced = (1.0 - 2.0 * (torch.rand(n, N) < 0.5).float())
                with torch.no_grad():
                    dec, _ = net.decode(yt, list(info), ones, dev)
                bits, logits = stepped_dec(net, yt, set(info.tolist()))
                assert np.array_equal(dec.numpy(), bits), "the stepped modules do not give decode()'s bits"
                _, flog = stepped_dec(net, torch.from_numpy(yf), set(info.tolist()), forced)
                _, f64 = X.decode64_dec(sd, yf, is_info, forced=forced.numpy())
                e_ref = float(np.abs(flog.astype(np.float64) - f64)[:, info].max())
                b64, l64 = X.decode64_dec(sd, y, is_info)
                cols = info
                with torch.no_grad():
                    fwd = net(torch.from_numpy(yf[:FWD_WORDS]), torch.ones(FWD_WORDS, N).long(), forced[:FWD_WORDS], dev)[3]
                out.update(y_forced=yf, forced=forced.numpy().astype(np.int8), forced_logits=flog.astype(np.float32),
                           fwd_logits=fwd[:, :, 0].numpy().astype(np.float32))
            else:
                with torch.no_grad():
                    dec, _ = net.decode(yt, list(info), ones, dev)
                    logits = net(yt, ones, None, dev)[3][:, :, 0].numpy()
                bits = dec[:, :, 0].numpy()
                assert np.array_equal(bits, np.sign(logits)), "decode() is not the sign of forward()'s logits"
                l64 = X.forward64_enc(sd, y)
                b64 = np.sign(l64)
                e_ref = float(np.abs(logits.astype(np.float64) - l64).max())
                cols = np.arange(N)
                out.update(fwd_logits=logits[:FWD_WORDS].astype(np.float32))
            tol = max(X.LOGIT_ATOL, 4.0 * e_ref)
            robust = np.abs(l64[:, cols]).min(1) >= 10 * tol
            assert robust.mean() >= 0.9, f"{name}: only {int(robust.sum())} of {n} words are robust -- change the seed"
            assert np.array_equal(bits[robust], b64[robust]), f"{name}: the reference's bits differ from float64 on a robust word"
            out.update(ref_bits=bits.astype(np.int8), ref_logits=logits.astype(np.float32), e_ref=e_ref)
            path = os.path.join(OUT, name + ".npz")
            stored = L <= STORE_WEIGHTS_UP_TO[model]
            if stored:
                np.savez_compressed(path, **out, **{"w." + k: v for k, v in sd.items()})
                stored = os.path.getsize(path) <= SIZE_LIMIT
            if not stored:
                np.savez_compressed(path, **out, w_seed=W_SEED,
                                    w_digest=np.frombuffer(weights_digest(sd).encode(), np.uint8))
            assert os.path.getsize(path) <= SIZE_LIMIT
            msgs = {tuple(r) for r in bits[:, info].tolist()}
            print(f"{name}: e_ref {e_ref:.2e}, robust {int(robust.sum())}/{n}, {len(msgs)} distinct decoded messages, "
                  f"weights {'stored' if stored else 'by seed'}, {os.path.getsize(path) / 1e6:.2f} MB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
