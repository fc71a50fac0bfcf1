"""Float64 restatement of XFormerEndToEndGPT.decode (models.py:398-423) and the GPT fixtures' loader.

decode64 is written from the semantics, not from the reference's code: at information position i the post-LN layer
stack runs on tokens 0 .. i, every token attending to every key <= i, and logit_i = Lin_Decoder(token i's output).
Two switches turn it into the negative controls of tests/test_gpt.py: ``causal`` (token t sees keys <= t only, which is
what a KV-cached decode computes) and ``no_table`` (the sinusoid buffer left out).
"""
import argparse
import math
import os

import numpy as np

from conftest import GOLDEN, weights_digest

E, H = 64, 8
LOGIT_ATOL = 2e-5
FIXTURES = ["gpt_polar_16_8_l1", "gpt_polar_32_16_l2", "gpt_polar_64_32_l2", "gpt_polar_32_16_l6", "gpt_polar_64_32_l6"]
DECISION_FIXTURES = FIXTURES[:3]
DEEP_FIXTURES = FIXTURES[1:]   # >= 2 layers: a causal decode differs from the reference's
INIT_SCALE = 3.0               # every 2-D parameter x 3 after the seeded default initialisation (gen_gpt.py)

def gelu64(x):
    import torch
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x / math.sqrt(2.0)))).numpy())


def layer_norm64(x, g, b):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + 1e-6) * g + b


def gpt_config(N, n_layers, embed_dim=E, n_head=H, max_len=None):
    return argparse.Namespace(N=N, max_len=N if max_len is None else max_len, embed_dim=embed_dim, n_head=n_head,
                              n_layers=n_layers, dropout=0.0, model="gpt")


def seeded_state_dict(N, n_layers, seed):
    """The fixtures' weights: this package's class under torch.manual_seed(seed) (the same parameter draws, in the
    same order, as the reference's class -- gen_gpt.py checks the digest against the reference's), 2-D parameters x 3."""
    import torch
    from neural_polar_decoder_amd.models import XFormerEndToEndGPT
    torch.manual_seed(seed)
    net = XFormerEndToEndGPT(gpt_config(N, n_layers))
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 2:
                p.mul_(INIT_SCALE)
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


_CACHE = {}


def fixture(name):
    """(npz, state dict as numpy arrays) -- loaded once per session and shared."""
    if name not in _CACHE:
        d = np.load(os.path.join(GOLDEN, name + ".npz"))
        keys = [str(k) for k in d["keys"]]
        if "w_seed" in d.files:
            sd = seeded_state_dict(int(d["N"]), int(d["n_layers"]), int(d["w_seed"]))
            assert weights_digest(sd) == bytes(d["w_digest"]).decode(), "regenerated GPT weights differ from the fixture's"
        else:
            sd = {k: np.asarray(d["w." + k]) for k in keys}
        _CACHE[name] = (d, sd)
    return _CACHE[name]


def tol_of(d):
    """max(2e-5, 4 e_ref): LOGIT_ATOL, or four times the reference's own fp32 error on these logits."""
    return max(LOGIT_ATOL, 4.0 * float(d["e_ref"]))


def decode64(sd, y, is_info, forced=None, causal=False, no_table=False):
    """(bits (B,N), logits (B,N)) in float64; logits 0 and bits +1 at frozen positions."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    y = np.asarray(y, np.float64)
    B, N = y.shape
    L = 1 + max(int(k.split(".")[2]) for k in w if k.startswith("Decoder.layer_stack."))
    d = E // H
    h = gelu64(y @ w["start_embed_layer.0.weight"].T + w["start_embed_layer.0.bias"])
    h = gelu64(h @ w["start_embed_layer.2.weight"].T + w["start_embed_layer.2.bias"])
    start = h @ w["start_embed_layer.4.weight"].T + w["start_embed_layer.4.bias"]
    pos_emb = w["pos_emb.weight"]
    table = w["Decoder.position_enc_auto.pos_table"][0]
    feed = np.ones((B, N)) if forced is None else np.asarray(forced, np.float64).copy()
    bits, logits = np.ones((B, N)), np.zeros((B, N))
    for i in range(N):
        if not is_info[i]:
            continue
        n = i + 1
        X = np.empty((B, n, E))
        X[:, 0] = start
        X[:, 1:] = feed[:, :i, None] * pos_emb[None, 1:n]
        if not no_table:
            X = X + table[None, :n]
        for l in range(L):
            p = f"Decoder.layer_stack.{l}."
            q = (X @ w[p + "slf_attn.w_qs.weight"].T).reshape(B, n, H, d).transpose(0, 2, 1, 3)
            k = (X @ w[p + "slf_attn.w_ks.weight"].T).reshape(B, n, H, d).transpose(0, 2, 1, 3)
            v = (X @ w[p + "slf_attn.w_vs.weight"].T).reshape(B, n, H, d).transpose(0, 2, 1, 3)
            s = (q / math.sqrt(d)) @ k.transpose(0, 1, 3, 2)
            if causal:
                s = np.where(np.tril(np.ones((n, n), bool))[None, None], s, -np.inf)
            s = np.exp(s - s.max(-1, keepdims=True))
            a = s / s.sum(-1, keepdims=True)
            o = (a @ v).transpose(0, 2, 1, 3).reshape(B, n, E)
            X = layer_norm64(o @ w[p + "slf_attn.fc.weight"].T + X, w[p + "slf_attn.layer_norm.weight"],
                             w[p + "slf_attn.layer_norm.bias"])
            f = gelu64(X @ w[p + "pos_ffn.w_1.weight"].T + w[p + "pos_ffn.w_1.bias"])
            X = layer_norm64(f @ w[p + "pos_ffn.w_2.weight"].T + w[p + "pos_ffn.w_2.bias"] + X,
                             w[p + "pos_ffn.layer_norm.weight"], w[p + "pos_ffn.layer_norm.bias"])
        lg = X[:, i] @ w["Lin_Decoder.weight"][0] + w["Lin_Decoder.bias"][0]
        logits[:, i] = lg
        bits[:, i] = np.sign(lg)
        if forced is None:
            feed[:, i] = bits[:, i]
    return bits, logits


_REF64 = {}


def forced64(name):
    """Float64 logits along the fixture's forced paths, computed once per session."""
    if name not in _REF64:
        d, sd = fixture(name)
        _REF64[name] = decode64(sd, d["y_forced"], d["is_info"], forced=d["forced"])[1]
    return _REF64[name]


_FREE64 = {}


def free64(name):
    """Float64 free decode (bits, logits) of the fixture's words, computed once per session."""
    if name not in _FREE64:
        d, sd = fixture(name)
        _FREE64[name] = decode64(sd, d["y"], d["is_info"])
    return _FREE64[name]


def build_net(name, device="cpu"):
    """This package's class holding the fixture's weights (strict load)."""
    import torch
    from neural_polar_decoder_amd.models import XFormerEndToEndGPT
    d, sd = fixture(name)
    net = XFormerEndToEndGPT(gpt_config(int(d["N"]), int(d["n_layers"])))
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(device).eval()
