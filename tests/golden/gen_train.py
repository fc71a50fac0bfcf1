#!/usr/bin/env python3
"""Record the reference's training decode (rnn_all.RNN_decoder.decode(net, True, y, gt, tfr), rnn_all.py:422-512) and
its gradients in float64 for tests/test_gru_train.py, by IMPORTING the reference (never copying it).  Run where the
reference is present:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_train.py --reference /path/to/reference

The reference runs under torch.set_default_dtype(torch.float64), so its own torch.ones / eye / zeros are float64.  Each
net is the reference's RNN_Model with PyTorch-default fp32 draws under a seed (fp32 values, held in float64).  Per
fixture and mode (teacher: tfr 1.0, student: tfr 0.0) the loss is

    MSE(decoded[:, info], gt[:, info]) + sum(decoded * gmat)

gmat a small recorded random matrix: under reverse_order with student forcing the written steps (ii in info) land on
the positions N-1-ii, which for Polar(16, 8) are all frozen, so the MSE term alone would leave every gradient zero.
Recorded: y, gt, info, gmat, the weights, and per mode decoded, the loss's gradient at decoded and every parameter's.
"""
import argparse
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import train_helper as T  # noqa: E402

B = 24
# name -> (F, layers, N, onehot, reverse_order, seed)
SPECS = {
    "train_gru_f32_l1_n16_rev": (32, 1, 16, False, True, 6101),
    "train_gru_f64_l2_n16_onehot": (64, 2, 16, True, False, 6102),
}
assert tuple(SPECS) == T.FIXTURES


def _import_reference(ref):
    if not os.path.isdir(ref):
        raise SystemExit("reference not present: fixtures can only be generated where it is")
    sys.path.insert(0, ref)
    ip = types.ModuleType("IPython")
    ip.display = None
    ip.get_ipython = lambda: None
    sys.modules.setdefault("IPython", ip)
    import rnn_all  # noqa: E402
    return rnn_all


def generate(rnn_m, name):
    F, layers, N, onehot, rev, seed = SPECS[name]
    K = N // 2
    rnn_m.args = argparse.Namespace(hard_decision=False, target_K=K, random_seed=42, loss_only=None, K=K, N=N,
                                    no_detach=False)
    torch.set_default_dtype(torch.float32)
    info = np.sort(np.asarray(rnn_m.get_code("Polar", "polar", N, K).info_inds, np.int64))
    torch.manual_seed(seed)
    net = rnn_m.RNN_Model("GRU", N + 1 + int(onehot), F, 1, layers, N, 0, 0, "selu", 0.0, False, out_linear_depth=1)
    sd = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}  # fp32 values
    net = net.double()
    torch.set_default_dtype(torch.float64)
    y, gt = T.make_words(B, N, seed)
    rng = np.random.default_rng(seed + 1)
    gmat = (0.05 / B) * rng.standard_normal((B, N))
    out = {"F": np.int64(F), "layers": np.int64(layers), "N": np.int64(N), "onehot": np.int64(onehot),
           "rev": np.int64(rev), "seed": np.int64(seed), "info": info, "y": y, "gt": gt, "gmat": gmat}
    out.update({"w." + k: v for k, v in sd.items()})
    dec = rnn_m.RNN_decoder("y_input", N, info.tolist(), onehot=onehot, reverse_order=rev)
    ti = torch.from_numpy(info)
    for mode, tfr in (("teacher", 1.0), ("student", 0.0)):
        net.zero_grad()
        decoded = dec.decode(net, True, torch.from_numpy(y).double(), torch.from_numpy(gt).double(), tfr)
        assert decoded.dtype == torch.float64 and net.training
        decoded.retain_grad()
        loss = torch.nn.functional.mse_loss(decoded[:, ti], torch.from_numpy(gt).double()[:, ti]) \
            + (decoded * torch.from_numpy(gmat)).sum()
        loss.backward()
        d = decoded.detach().numpy()
        assert np.all(d != 0.0), "a decoded value was exactly 0"
        out[mode + ".decoded"] = d
        out[mode + ".gout"] = decoded.grad.numpy().copy()
        for k, p in net.named_parameters():
            assert float(p.grad.norm()) > 0.0, (name, mode, k)
            out[f"{mode}.g.{k}"] = p.grad.numpy().copy()
    torch.set_default_dtype(torch.float32)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000 * 1024


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory that holds the reference's rnn_all.py")
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    m = _import_reference(a.reference)
    for n in (a.names or SPECS):
        generate(m, n)
