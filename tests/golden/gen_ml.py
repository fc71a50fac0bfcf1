#!/usr/bin/env python3
"""Generate the ML / bitwise-MAP fixtures tests/golden/ml_*.npz by IMPORTING the reference (as gen_golden.py does;
never copying it).  CPU only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ml.py

Reference code run:
  utils.dec2bitarray -> all_message_bits                               utils.py:170-192, run_models.py:1349-1354
  PolarCode.encode_plotkin / PAC.pac_encode of all_message_bits        run_models.py:1355, :1364
  the inline ML block  b_noisy.repeat, (b_noisy - b_codebook).pow(2).sum(2).argmin(1)   run_models.py:348-351
  PolarCode.bitwise_MAP (decisions; its fp32 logsumexp arithmetic for the LLR error)     polar.py:879-899
  PolarCode.channel / PAC.channel                                      polar.py:201-207, pac_code.py:226-231

Per code, 64 words at each of 0, 2 and 4 dB.  Stored: y, snr, scale = fl32(2 / sigma^2), info, g, seed, the reference's
ML index, (Polar) the reference's bitwise_MAP decisions, the float64 LLRs of a = scale * y, and the largest error of
the reference's own fp32 LLR arithmetic against float64.

Preconditions, asserted; the seed is stepped until they hold:
  * on every stored word the reference's index equals the float64 argmax of the correlations,
  * the float64 top-two margin is at least 4 eps(y), eps(y) = 2 N 2^-24 sum_j |y_j|,
  * at most 1 % of the LLRs of an SNR point have |LLR64| <= delta(y),
    delta(y) = 2 [(N + 4) 2^-24 sum_j |a_j| + (2^(K-1) + 8) 2^-24],
  * the reference's decisions agree with sign(LLR64) on all the others.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, ns, pac_m, polar_code, save, utils_m  # noqa: E402  (imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SNRS = (0.0, 2.0, 4.0)
PER = 64
U = 2.0 ** -24

CODES = [("polar", 8, 2, 0), ("polar", 16, 8, 0), ("polar", 32, 16, 0), ("polar", 64, 12, 0),
         ("pac", 32, 10, 53), ("pac", 16, 5, 91)]


def eps_of(y, N):
    return 2.0 * N * U * np.abs(y.astype(np.float64)).sum(1)


def delta_of(a, N, K):
    return 2.0 * ((N + 4) * U * np.abs(a).sum(1) + (2.0 ** (K - 1) + 8) * U)


def lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return np.log(np.exp(x - m).sum(axis=axis)) + np.squeeze(m, axis)


def build(kind, N, K, g):
    if kind == "polar":
        code = polar_code(N, K)
        enc = code.encode_plotkin
        info = np.asarray(code.info_positions, np.int64)
    else:
        code = pac_m.PAC(ns(target_K=K), N, K, g)
        enc = lambda m: code.pac_encode(m, scheme="RM")  # noqa: E731
        enc(torch.ones(1, K))
        info = np.asarray(code.B, np.int64)
    amb = torch.from_numpy(np.array([utils_m.dec2bitarray(i, K) for i in range(2 ** K)]))
    amb = 1 - 2 * amb.float()
    codebook = enc(amb)
    return code, enc, info, amb, codebook


def try_seed(kind, N, K, g, seed, code, enc, amb, codebook):
    cb64 = codebook.numpy().astype(np.float64)
    ys, snrs, idxs, decs, llrs = [], [], [], [], []
    ref_err = 0.0
    for si, snr in enumerate(SNRS):
        torch.manual_seed(seed + si)
        msg = 1.0 - 2.0 * torch.randint(0, 2, (PER, K)).float()
        y = code.channel(enc(msg), snr)
        # the reference's ML arithmetic (run_models.py:348-351), 8 words at a time to bound the repeat's memory
        idx = []
        for o in range(0, PER, 8):
            b_noisy = y[o:o + 8].unsqueeze(1).repeat(1, 2 ** K, 1)
            b_codebook = codebook.repeat(b_noisy.shape[0], 1, 1)
            idx.append((b_noisy - b_codebook).pow(2).sum(dim=2).argmin(dim=1))
        idx = torch.cat(idx).numpy()
        y64 = y.numpy().astype(np.float64)
        corr = y64 @ cb64.T
        if not np.array_equal(corr.argmax(1), idx):
            return None, "reference index != float64 argmax"
        top2 = np.partition(corr, -2, axis=1)[:, -2:]
        if not np.all(top2[:, 1] - top2[:, 0] >= 4 * eps_of(y.numpy(), N)):
            return None, "margin < 4 eps"
        scale = np.float32(2 / utils_m.snr_db2sigma(snr) ** 2)
        a = np.float64(scale) * y64
        ca = a @ cb64.T
        plus = amb.numpy() == 1.0                                   # (2^K, K): bit_k(i) = 0
        llr = np.stack([lse(ca[:, plus[:, k]], 1) - lse(ca[:, ~plus[:, k]], 1) for k in range(K)], axis=1)
        near = np.abs(llr) <= delta_of(a, N, K)[:, None]
        if near.mean() > 0.01:
            return None, "more than 1 % of LLRs within delta of 0"
        # the reference's fp32 LLR arithmetic (polar.py:881, 891-894)
        ne = torch.from_numpy(np.float32(scale) * y.numpy())
        for k in range(K):
            d1 = torch.logsumexp(torch.matmul(codebook[amb[:, k] == 1.], ne.T).T, -1)
            d2 = torch.logsumexp(torch.matmul(codebook[amb[:, k] == -1.], ne.T).T, -1)
            ref_err = max(ref_err, float(np.abs((d1 - d2).numpy().astype(np.float64) - llr[:, k]).max()))
        if kind == "polar":
            dec = code.bitwise_MAP(y, "cpu", snr).numpy()
            want = np.where(llr >= 0, 1.0, -1.0)
            if not np.array_equal(dec[~near], want[~near]):
                return None, "reference decisions differ from float64 away from 0"
            decs.append(dec.astype(np.int8))
        ys.append(y.numpy()); snrs.append(np.full(PER, snr)); idxs.append(idx.astype(np.int32)); llrs.append(llr)
    out = dict(y=np.concatenate(ys), snr=np.concatenate(snrs), idx=np.concatenate(idxs), llr64=np.concatenate(llrs),
               ref_llr_err=np.float64(ref_err), scale=np.array([np.float32(2 / utils_m.snr_db2sigma(s) ** 2) for s in SNRS]),
               seed=np.int64(seed), N=np.int64(N), K=np.int64(K), g=np.int64(g), pac=np.int64(kind == "pac"))
    if decs:
        out["map_dec"] = np.concatenate(decs)
    return out, None


def main():
    torch.set_num_threads(8)
    for kind, N, K, g in CODES:
        code, enc, info, amb, codebook = build(kind, N, K, g)
        seed = 7000 + 100 * N + K
        while True:
            out, why = try_seed(kind, N, K, g, seed, code, enc, amb, codebook)
            if out is not None:
                break
            print(f"{kind}({N},{K}) seed {seed}: {why}; stepping the seed")
            seed += 10
        out["info"] = info
        name = f"ml_{kind}_{N}_{K}.npz"
        save(name, **out)
        size = os.path.getsize(os.path.join(OUT, name))
        print(f"  {name}: {size} bytes, reference fp32 LLR error vs float64 <= {out['ref_llr_err']:.3g}")
        assert size < 100 * 1024


if __name__ == "__main__":
    main()
