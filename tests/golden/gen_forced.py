#!/usr/bin/env python3
"""Record the reference's genie decode (rnn_all.RNN_decoder.decode with gt and loss_inds, rnn_all.py:514-561) for the
forced-path tests, by IMPORTING the reference (never copying it).  Run where the reference is present:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_forced.py

Each fixture is data: a net (the reference's RNN_Model under torch.manual_seed(seed), every parameter times g), 64 words
y = +-1 + 0.8 N(0, 1), a gt whose frozen positions hold one of {-1, +1, 0, -0.3, 2.5}, and what
RNN_decoder.decode(net, False, y, gt=gt, loss_inds=info) returned, with the logits of every step (a forward hook on
net.linear).  They pin to the reference itself what tests/forced_helper.py restates: which entry of gt survives under
reverse_order, that decoded keeps gt's raw values, that sign(decoded) is fed back, and that 0 selects one-hot column 0.
Weights are stored, except where they would take the file past 100 KB: then the seed and a digest are stored and the test
regenerates them with this package's RNN_Model (the same parameter draws) and checks the digest.
"""
import argparse
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import forced_helper as H  # noqa: E402

torch.set_num_threads(8)
B = 64
# name -> (cell, F, layers, N, onehot, reverse_order, g, seed)
SPECS = {
    "forced_gru_f32_l1_n16_rev": ("GRU", 32, 1, 16, False, True, 4.0, 5101),
    "forced_gru_f64_l2_n32_onehot": ("GRU", 64, 2, 32, True, False, 4.0, 5102),
    "forced_lstm_f32_l2_n16_rev": ("LSTM", 32, 2, 16, True, True, 4.0, 5103),
}
assert tuple(SPECS) == H.FIXTURES


def _import_reference():
    if not os.path.isdir(REF):
        raise SystemExit("reference not present: fixtures can only be generated in the build container")
    sys.path.insert(0, REF)
    ip = types.ModuleType("IPython")
    ip.display = None
    ip.get_ipython = lambda: None
    sys.modules.setdefault("IPython", ip)
    import rnn_all  # noqa: E402
    return rnn_all


def generate(rnn_m, name):
    cell, F, layers, N, onehot, rev, g, seed = SPECS[name]
    K = N // 2
    rnn_m.args = argparse.Namespace(hard_decision=False, target_K=K, random_seed=42, loss_only=None, K=K, N=N,
                                    no_detach=False)
    info = np.sort(np.asarray(rnn_m.get_code("Polar", "polar", N, K).info_inds, np.int64))
    assert np.array_equal(info, H.info_set(N))
    torch.manual_seed(seed)
    net = rnn_m.RNN_Model(cell, N + 1 + int(onehot), F, 1, layers, N, 0, 0, "selu", 0.0, False, out_linear_depth=1)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(g)
    net.eval()
    rng = np.random.default_rng(seed)
    y = (np.where(rng.random((B, N)) < 0.5, -1.0, 1.0) + 0.8 * rng.standard_normal((B, N))).astype(np.float32)
    gt = np.where(rng.random((B, N)) < 0.5, -1.0, 1.0).astype(np.float32)
    frozen = np.setdiff1d(np.arange(N), info)
    gt[:, frozen] = np.asarray(H.FROZEN_VALUES, np.float32)[rng.integers(0, len(H.FROZEN_VALUES), (B, frozen.size))]
    rec = []
    hook = net.linear.register_forward_hook(lambda m, i, o: rec.append(o.detach().clone()))
    dec = rnn_m.RNN_decoder("y_input", N, info.tolist(), onehot=onehot, reverse_order=rev)
    decoded = dec.decode(net, False, torch.from_numpy(y), gt=torch.from_numpy(gt), loss_inds=info.tolist())
    hook.remove()
    logits = torch.stack([r.view(-1) for r in rec], 1).numpy()
    assert logits.shape == (B, N) and np.all(logits != 0.0), "a logit was exactly 0"
    sd = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    out = {"cell": np.bytes_(cell), "F": np.int64(F), "layers": np.int64(layers), "N": np.int64(N),
           "onehot": np.int64(onehot), "rev": np.int64(rev), "g": np.float64(g), "seed": np.int64(seed), "info": info,
           "y": y, "gt": gt, "decoded": decoded.numpy(), "logits": logits, "w_digest": np.bytes_(H.weights_digest(sd))}
    if sum(v.nbytes for v in sd.values()) + 4 * y.nbytes <= 90 * 1024:
        out.update({"w." + k: v for k, v in sd.items()})
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; weights", "stored" if "w.linear.weight" in out else "by seed",
          "max |logit|", float(np.abs(logits).max()))
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    m = _import_reference()
    for n in (sys.argv[1:] or SPECS):
        generate(m, n)
