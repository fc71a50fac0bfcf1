"""Writes tests/golden/pac_scl_*.npz: PAC SC-List decoding composed from the reference's own functions.

    python tests/golden/gen_pac_scl.py /path/to/reference

The reference has no PAC list decoder.  This composes PolarCode.scl_decode's list handling (polar.py:793-876,
use_CRC=False: fork in list order [keep.., flip..], torch.topk pruning kept in ascending order, final choice by
distance to polar_encode(u)) with pac_sc_decode's leaf step (pac_code.py:534-573: conv1bTrans_batch on the path's
convolution state, the z_inds / o_inds rule for zero decisions), calling the reference's updateLLR,
updatePartialSums, conv1bTrans_batch, polar_encode and torch.topk.  Only data is stored: y, snr, L, g, info,
msg_hat (= v_hat[:, info]), u_hat, leaf (the chosen path's leaf LLRs).

Rows of each file: random words at 0 .. 4 dB; grid-valued words (y in {-1.5 .. 1.5}, snr 1.0: many metric ties,
exactly representable distances); a few crafted rows with exact zeros.  A random row whose two best list
candidates are closer, in float64, than fp32 summation order could separate is dropped (at most 1 % of a file).
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
#        N    K    g   Ls            random rows per SNR, grid rows
CASES = [(8, 4, 13, (4,), 40, 60),
         (16, 8, 13, (2,), 40, 60),
         (32, 16, 53, (1, 3, 4, 8), 40, 60),
         (64, 22, 91, (4,), 24, 40),
         (64, 32, 91, (8,), 24, 40),
         (128, 64, 91, (4, 8), 12, 20),
         (256, 128, 91, (4, 8), 6, 10)]
SNRS = (0.0, 1.0, 2.0, 3.0, 4.0)
GRID = np.array([-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5], np.float32)


def pac_scl(pac, y, snr, L, snr_db2sigma):
    """(leaf LLRs, v_hat[:, B], u_hat) of the chosen path and every final candidate's codeword (S, bs, N)."""
    N, n = pac.N, pac.n
    g = pac.g_array
    m = len(g) - 1
    Bset = set(int(i) for i in pac.B)
    sigma = snr_db2sigma(snr)
    llrs = (2 / sigma ** 2) * y
    bs = y.shape[0]
    u_list = torch.zeros(1, bs, N)
    v_list = torch.zeros(1, bs, N)
    cs_list = torch.ones(1, bs, m)
    la, ps = pac.define_partial_arrays(llrs)
    la_list = la.unsqueeze(0)
    ps_list = ps.unsqueeze(0)
    met = torch.zeros(1, bs)
    for ii in range(N):
        ls = la_list.shape[0]
        la, _ = pac.updateLLR(ii, la_list.reshape(-1, n + 1, N).clone(), ps_list.reshape(-1, n + 1, N))
        leaf = la[:, 0, ii]
        cs = cs_list.reshape(-1, m)
        u0, cs0 = pac.conv1bTrans_batch(torch.ones(ls * bs), cs, g)
        u1, cs1 = pac.conv1bTrans_batch(-torch.ones(ls * bs), cs, g)
        if ii not in Bset:
            pen = leaf.abs() * (leaf.sign() != u0).float()
            u_list[:, :, ii] = u0.reshape(ls, bs)
            v_list[:, :, ii] = 1.
            cs_list = cs0.reshape(ls, bs, m)
            ps = pac.updatePartialSums(ii, u_list.reshape(-1, N), ps_list.reshape(-1, n + 1, N).clone())
            la_list = la.reshape(ls, bs, n + 1, N)
            ps_list = ps.reshape(ls, bs, n + 1, N)
            met = met + pen.reshape(ls, bs)
            continue
        s = leaf.sign()

        def child(uc):
            z = u0 == uc
            o = u1 == uc
            v = torch.zeros_like(uc)
            v[z] = 1.
            v[o] = -1.
            c = cs.clone()
            c[z] = cs0[z]
            c[o] = cs1[o]
            return v, c

        vk, ck = child(s)
        vf, cf = child(-s)
        u_list = torch.vstack([u_list, u_list])
        v_list = torch.vstack([v_list, v_list])
        u_list[:ls, :, ii] = s.reshape(ls, bs)
        u_list[ls:, :, ii] = (-s).reshape(ls, bs)
        v_list[:ls, :, ii] = vk.reshape(ls, bs)
        v_list[ls:, :, ii] = vf.reshape(ls, bs)
        cs_list = torch.vstack([ck.reshape(ls, bs, m), cf.reshape(ls, bs, m)])
        la_list = torch.vstack([la.reshape(ls, bs, n + 1, N)] * 2)
        ps_list = pac.updatePartialSums(ii, u_list.reshape(-1, N),
                                        torch.vstack([ps_list, ps_list]).reshape(-1, n + 1, N).clone()
                                        ).reshape(2 * ls, bs, n + 1, N)
        met = torch.vstack([met, met + leaf.abs().reshape(ls, bs)])
        if la_list.shape[0] > L:
            _, inds = torch.topk(-met, L, 0)
            si, _ = torch.sort(inds, 0)
            ar = torch.arange(bs)
            la_list, ps_list, met = la_list[si, ar], ps_list[si, ar], met[si, ar]
            u_list, v_list, cs_list = u_list[si, ar], v_list[si, ar], cs_list[si, ar]
    ls = la_list.shape[0]
    cw = pac.polar_encode(u_list.reshape(-1, N)).reshape(ls, bs, N)
    # first minimum of the sequential fp32 sum, as the kernels and the test restatement compute it
    dist = torch.zeros(ls, bs)
    for k in range(N):
        dd = cw[:, :, k] - y[:, k].unsqueeze(0)
        dist = dist + dd * dd
    inds = torch.zeros(bs, dtype=torch.int64)
    bd = dist[0].clone()
    for j in range(1, ls):
        lt = dist[j] < bd
        inds[lt] = j
        bd = torch.where(lt, dist[j], bd)
    vec = ((cw - y.unsqueeze(0)) ** 2).sum(2).argmin(0)   # the reference's own reduction (polar.py:868-874)
    ar = torch.arange(bs)
    return la_list[inds, ar, 0, :], v_list[inds, ar][:, pac.B], u_list[inds, ar], cw, (vec != inds)


def separable(cw, y):
    """Rows whose two best distinct candidates differ, in float64, by more than fp32 summation could blur."""
    S, bs, N = cw.shape
    if S == 1:
        return np.ones(bs, bool)
    d = ((cw.double() - y.double().unsqueeze(0)) ** 2).sum(2).numpy()
    d = np.sort(d, 0)
    return d[1] - d[0] > 2 * (N + 4) * 2.0 ** -24 * d[1]


def crafted(N, rng):
    """Rows with exact zeros: leaf LLRs that are exactly 0 reach information positions (u = v = 0, no state advance)."""
    base = np.where(rng.integers(0, 2, (8, N)) == 1, -1.0, 1.0).astype(np.float32) * rng.choice(
        np.array([0.5, 1.0, 1.5], np.float32), (8, N))
    base[0] = 0.0
    base[1, :N // 2] = 0.0
    base[2, N // 2:] = 0.0
    base[3, 0::2] = 0.0
    base[4, 1::2] = 0.0
    base[5, N // 4:N // 2] = 0.0
    base[6, rng.random(N) < 0.5] = 0.0
    base[7, 3 * N // 4:] = 0.0
    return base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="directory of the reference project")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from pac_code import PAC
    from utils import snr_db2sigma
    for N, K, g, Ls, nrand, ngrid in CASES:
        for L in Ls:
            torch.manual_seed(1000 * N + 10 * K + L)
            rng = np.random.default_rng(1000 * N + 10 * K + L)
            pac = PAC(argparse.Namespace(hard_decision=True), N, K, g)
            info = np.asarray(pac.B).copy()
            rows = {k: [] for k in ("y", "snr", "msg_hat", "u_hat", "leaf")}
            total = dropped = 0

            def run(y, snr, random_rows):
                nonlocal total, dropped
                leaf, vh, uh, cw, differs = pac_scl(pac, y, snr, L, snr_db2sigma)
                keep = np.ones(y.shape[0], bool)
                if random_rows:
                    keep = separable(cw, y)
                    total += keep.size
                    dropped += int((~keep).sum())
                else:
                    assert not bool(differs.any()), "exactly representable distances: every reduction order agrees"
                assert not bool(differs.numpy()[keep].any()), "a kept row depends on the summation order"
                rows["y"].append(y.numpy()[keep])
                rows["snr"].append(np.full(int(keep.sum()), snr, np.float32))
                rows["msg_hat"].append(vh.numpy()[keep])
                rows["u_hat"].append(uh.numpy()[keep])
                rows["leaf"].append(leaf.numpy()[keep])

            for snr in SNRS:
                msg = 1 - 2 * torch.randint(0, 2, (nrand, K)).float()
                run(pac.channel(pac.pac_encode(msg), snr), snr, True)
            run(torch.from_numpy(GRID[rng.integers(0, GRID.size, (ngrid, N))]), 1.0, False)
            run(torch.from_numpy(crafted(N, rng)), 1.0, False)
            assert dropped * 100 <= total, (N, K, L, dropped, total)
            out = {k: np.concatenate(v).astype(np.float32) for k, v in rows.items()}
            zero = np.float32(0.0)
            out = {k: v + zero for k, v in out.items()}  # -0.0 -> +0.0
            path = os.path.join(HERE, f"pac_scl_{N}_{K}_L{L}.npz")
            np.savez_compressed(path, L=np.int32(L), g=np.int32(g), info=info.astype(np.int64), **out)
            print(f"{os.path.basename(path)}: {out['y'].shape[0]} rows, {dropped} of {total} random rows dropped, "
                  f"{int((out['u_hat'] == 0).any(1).sum())} rows with a zero decision, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
