#!/usr/bin/env python3
"""GPT transformer fixtures: tests/golden/gpt_polar_*.npz, from the reference's XFormerEndToEndGPT (models.py:340-423).

Run in the build container only (``/root/reference`` does not exist on the GPU box; without it the script says so and
writes nothing):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_gpt.py

models.py imports IPython, which is not installed: a stub module stands in for it.

Weights.  torch.manual_seed(11), the reference's class with PyTorch's default initialisation, then every 2-D parameter
x 3: at the default scale the decisions ignore y (one distinct decoded word in 96).  Fixtures of up to 2 layers store
the state dict; the 6-layer ones would pass the size limit of a committed file, so they store the seed and a sha256 of
the state dict, and tests/gpt_helper.py regenerates the weights with this package's class (same draws, same order --
checked here against the reference's for every fixture).

Words.  Polar(N, K) codewords at 2 dB (torch.manual_seed(seed_y); msg = 1 - 2 (rand < 0.5); y = encode(msg) + sigma
randn); forced paths are random +-1 words of N bits on a second set of codewords.

Stored per fixture: the state-dict key list; y, the reference's decode() bits and the fp32 logits behind them (its own
modules, stepped as decode steps them, and checked to give decode()'s bits); y_forced, forced and the fp32 logits along
the forced paths; e_ref = max |reference fp32 - float64 restatement| over the information logits of the forced paths.
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
CASES = [dict(name="gpt_polar_16_8_l1", N=16, K=8, L=1, n=96, nf=96, seed_y=101),
         dict(name="gpt_polar_32_16_l2", N=32, K=16, L=2, n=96, nf=96, seed_y=102),
         dict(name="gpt_polar_64_32_l2", N=64, K=32, L=2, n=48, nf=48, seed_y=103),
         dict(name="gpt_polar_32_16_l6", N=32, K=16, L=6, n=96, nf=96, seed_y=104),
         dict(name="gpt_polar_64_32_l6", N=64, K=32, L=6, n=48, nf=32, seed_y=105)]
STORE_WEIGHTS_UP_TO = 2  # layers


def words(N, K, info, n, seed, O):
    torch.manual_seed(seed)
    msg = 1.0 - 2.0 * (torch.rand(n, K) < 0.5).float()
    x = torch.from_numpy(O.encode_plotkin(msg.numpy(), N, info))
    sigma = 10 ** (-2.0 / 20)
    return (x + sigma * torch.randn(x.shape)).numpy().astype(np.float32)


def stepped(net, y, info, forced=None):
    """The reference's modules stepped as its decode steps them (models.py:398-423), keeping the logits."""
    dev = torch.device("cpu")
    B, N = y.shape
    with torch.no_grad():
        seq = torch.ones((B, N, net.embed_dim))
        seq[:, 0] = net.start_embed_layer(y)
        tri = torch.tril(torch.ones((1, N, N))).bool()
        bits, logits = torch.ones((B, N)), torch.zeros((B, N))
        for i in range(N):
            nb = torch.ones(B)
            if i in info:
                lg = net.Lin_Decoder(net.Decoder(seq, tri[:, i, :].unsqueeze(1), dev))[:, i, 0]
                logits[:, i] = lg
                nb = lg.sign()
            bits[:, i] = nb
            if i < N - 1:
                feed = nb if forced is None else forced[:, i]
                seq[:, i + 1] = feed.unsqueeze(1) * net.pos_emb(torch.tensor(i + 1)).unsqueeze(0)
    return bits.numpy(), logits.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    if not os.path.isdir(REF):
        print(f"gen_gpt: {REF} is absent -- nothing generated")
        return 0
    for p in (ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    from gpt_helper import INIT_SCALE, decode64, gpt_config, seeded_state_dict
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
    for c in CASES:
        if a.only and a.only != c["name"]:
            continue
        N, K, L = c["N"], c["K"], c["L"]
        info = np.sort(np.asarray(polar_info_positions(N, K, "polar", None))).astype(np.int64)
        is_info = np.zeros(N, np.uint8)
        is_info[info] = 1
        torch.manual_seed(W_SEED)
        net = R.XFormerEndToEndGPT(gpt_config(N, L)).eval()
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 2:
                    p.mul_(INIT_SCALE)
        sd = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
        ours = seeded_state_dict(N, L, W_SEED)
        assert list(ours) == list(sd) and weights_digest(ours) == weights_digest(sd), "this package's class draws differently"
        y = words(N, K, info, c["n"], c["seed_y"], O)
        yf = words(N, K, info, c["nf"], c["seed_y"] + 1000, O)
        torch.manual_seed(c["seed_y"] + 2000)
        forced = (1.0 - 2.0 * (torch.rand(c["nf"], N) < 0.5).float())
        with torch.no_grad():
            dec, _ = net.decode(torch.from_numpy(y), list(info), torch.ones(c["n"], N).bool(), torch.device("cpu"))
        bits, logits = stepped(net, torch.from_numpy(y), set(info.tolist()))
        assert np.array_equal(dec.numpy(), bits), "the stepped modules do not give decode()'s bits"
        _, flog = stepped(net, torch.from_numpy(yf), set(info.tolist()), forced)
        _, f64 = decode64(sd, yf, is_info, forced=forced.numpy())
        e_ref = float(np.abs(flog.astype(np.float64) - f64)[:, info].max())
        out = dict(N=N, K=K, n_layers=L, info=info, is_info=is_info, keys=np.array(list(sd)), y=y,
                   ref_bits=bits.astype(np.int8), ref_logits=logits.astype(np.float32), y_forced=yf,
                   forced=forced.numpy().astype(np.int8), forced_logits=flog.astype(np.float32), e_ref=e_ref,
                   w_scale=INIT_SCALE)
        if L <= STORE_WEIGHTS_UP_TO:
            out.update({"w." + k: v for k, v in sd.items()})
        else:
            out.update(w_seed=W_SEED, w_digest=np.frombuffer(weights_digest(sd).encode(), np.uint8))
        path = os.path.join(OUT, c["name"] + ".npz")
        np.savez_compressed(path, **out)
        msgs = {tuple(r) for r in bits[:, info].tolist()}
        print(f"{c['name']}: e_ref {e_ref:.2e}, {len(msgs)} distinct decoded messages in {c['n']}, "
              f"{os.path.getsize(path) / 1e6:.2f} MB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
