#!/usr/bin/env python3
"""Records tests/golden/conv_train_64_e16.npz from the reference's own convNet (models.py:691-767) in training mode on
the CPU: N = 64, embed 16, B = 6, weights conftest.conv_weights_from_seed(16, 64, SEED).

    python tests/golden/gen_conv_train.py /path/to/reference

Two modes, each in fp32 and in float64 (net.double()):
  plain.  config.dropout = 0
  drop.   config.dropout = 0.25, the Dropout layer's draw replaced by a fixed multiplier (0 or 1 / 0.75) through a
          forward hook, so the recorded numbers do not depend on torch's random stream
Recorded once: w.* (every parameter but layersFin.0.weight, which the seed reproduces; its float64 sum is kept as
w0sum).  Recorded per mode: y, gout, [drop], logits32 / logits64 and the gradients of sum(gout * logits), g32.* / g64.*.  The gradient of
layersFin.0.weight (256 x 1024, rank <= 6) is recorded as its rows ROWS (`layersFin.0.weight.rows`) and as proj^T dW
(`layersFin.0.weight.proj`, proj = PCG64(SEED + 2).standard_normal(256)), which weighs every row.

The reference is read here only; no test reads it.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from conftest import conv_weights_from_seed  # noqa: E402

SEED, N, E, B = 8001, 64, 16, 6
ROWS = np.arange(5, 256, 64)


def fc0_proj():
    return np.random.default_rng(SEED + 2).standard_normal(4 * N)


def record(models, sd, y, gout, drop, dtype):
    cfg = types.SimpleNamespace(embed_dim=E, max_len=N, N=N, dont_use_bias=False, dropout=0.0 if drop is None else 0.25)
    net = models.convNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(dtype).train()
    if drop is not None:
        mult = torch.as_tensor(drop, dtype=dtype)
        net.dropout.register_forward_hook(lambda mod, inp, out: inp[0] * mult)
    yt = torch.as_tensor(y, dtype=dtype)
    logits = net(yt, torch.ones(B, N), None, "cpu")[3].squeeze(-1)
    (logits * torch.as_tensor(gout, dtype=dtype)).sum().backward()
    grads = {}
    for k, p in net.named_parameters():
        g = p.grad.detach().numpy().copy()
        if k == "layersFin.0.weight":
            grads[k + ".rows"] = g[ROWS]
            grads[k + ".proj"] = (fc0_proj().astype(g.dtype) @ g) if dtype == torch.float64 else \
                (fc0_proj() @ g.astype(np.float64)).astype(np.float32)
        else:
            grads[k] = g
    return logits.detach().numpy().copy(), grads


def main():
    ref = sys.argv[1]
    if not os.path.isdir(ref):
        raise SystemExit("reference not present: fixtures can only be generated where it is")
    sys.path.insert(0, ref)
    ip = types.ModuleType("IPython")  # models.py imports IPython, which is not installed: a stub stands in
    ip.display = None
    ip.version_info = (8, 30, 0)
    ip.get_ipython = lambda: None
    sys.modules.setdefault("IPython", ip)
    import models  # the reference's
    sd = conv_weights_from_seed(E, N, SEED)
    rng = np.random.default_rng(SEED + 1)
    out = {}
    for mode in ("plain", "drop"):
        y = (np.where(rng.random((B, N)) < 0.5, -1.0, 1.0) + 0.8 * rng.standard_normal((B, N))).astype(np.float32)
        gout = rng.standard_normal((B, N)).astype(np.float32)
        drop = ((rng.random((B, N)) >= 0.25) / 0.75).astype(np.float32) if mode == "drop" else None
        l32, g32 = record(models, sd, y, gout, drop, torch.float32)
        l64, g64 = record(models, sd, y, gout, drop, torch.float64)
        p = mode + "."
        out.update({p + "y": y, p + "gout": gout, p + "logits32": l32, p + "logits64": l64})
        if drop is not None:
            out[p + "drop"] = drop
        out.update({p + "g32." + k: v for k, v in g32.items()})
        out.update({p + "g64." + k: v for k, v in g64.items()})
    out["w0sum"] = np.float64(sd["layersFin.0.weight"].astype(np.float64).sum())
    out.update({"w." + k: v for k, v in sd.items() if k != "layersFin.0.weight"})
    path = os.path.join(HERE, "conv_train_64_e16.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
