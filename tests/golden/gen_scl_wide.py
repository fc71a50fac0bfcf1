"""Writes tests/golden/widelist_polar_*.npz and widelist_pac_*.npz: SC-List decoding with 9 .. 32 paths.

    python tests/golden/gen_scl_wide.py [polar] [pac]

Needs the reference project where gen_golden.py looks for it.  Polar files hold the reference's own
PolarCode.scl_decode(y, snr, L, use_CRC=False) (polar.py:793-876); PAC files hold the composition of the reference's
functions that gen_pac_scl.py describes (its pac_scl), which takes any L.  Only data is stored.

Rows follow the existing list fixtures: random words at 0 .. 4 dB, grid-valued words (many metric ties at the pruning
boundary, exact zeros) and crafted rows with exact zeros, at the row counts those fixtures use at each N (the
N = 8 and N = 256 Polar files: 64 and 4 random rows per SNR, one pass of grid and crafted rows).  PAC: a random row
whose two best final candidates are closer, in float64, than fp32 summation order could separate is dropped, at most
1 % of a file.  Every file stays below the largest scl_*.npz (128,462 bytes).
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402  (imports the reference)
import gen_pac_scl as GP  # noqa: E402

MAX_BYTES = 128462
#        N    K    g   Ls        Polar: random rows per SNR, grid rows | PAC: random rows per SNR, grid rows
CASES = [(8, 4, 13, (32,), 64, 64, 40, 60),
         (16, 8, 13, (16,), 64, 64, 40, 60),
         (32, 16, 53, (12, 32), 64, 64, 40, 60),
         (64, 32, 91, (16,), 24, 24, 24, 40),
         (128, 64, 91, (32,), 8, 8, 12, 20),
         (256, 128, 91, (32,), 4, 4, 6, 10)]
SNRS = (0.0, 1.0, 2.0, 3.0, 4.0)


def finish(path, **arrs):
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (path, size)
    return size


def gen_polar():
    for N, K, _, Ls, per, ngrid, _, _ in CASES:
        for L in Ls:
            code = GG.polar_code(N, K)
            torch.manual_seed(3000 + N + K + L)
            rng = np.random.default_rng(3000 + N + K + L)
            ys, snrs, leafs, hats = [], [], [], []

            def run(y, snr):
                leaf, hat = code.scl_decode(y, float(snr), L, use_CRC=False)
                ys.append(y.numpy())
                snrs.append(np.full(y.shape[0], snr))
                leafs.append(leaf.numpy())
                hats.append(hat.numpy())

            for snr in SNRS:
                msg = 1.0 - 2.0 * torch.randint(0, 2, (per, K)).float()
                run(code.channel(code.encode_plotkin(msg), float(snr)), snr)
            run(torch.from_numpy(np.concatenate([GG.tie_rows(N, rng, ngrid), GG.crafted_rows(N, rng)])), 1.0)
            path = os.path.join(HERE, f"widelist_polar_{N}_{K}_L{L}.npz")
            size = finish(path, y=np.concatenate(ys), snr=np.concatenate(snrs), leaf=np.concatenate(leafs),
                          msg_hat=np.concatenate(hats), info=np.asarray(code.info_positions, np.int64), L=np.int64(L))
            print(f"{os.path.basename(path)}: {sum(y.shape[0] for y in ys)} rows, {size} bytes", flush=True)


def gen_pac():
    from pac_code import PAC
    from utils import snr_db2sigma
    for N, K, g, Ls, _, _, nrand, ngrid in CASES:
        for L in Ls:
            torch.manual_seed(1000 * N + 10 * K + L)
            rng = np.random.default_rng(1000 * N + 10 * K + L)
            pac = PAC(argparse.Namespace(hard_decision=True), N, K, g)
            info = np.asarray(pac.B).copy()
            rows = {k: [] for k in ("y", "snr", "msg_hat", "u_hat", "leaf")}
            total = dropped = 0

            def run(y, snr, random_rows):
                nonlocal total, dropped
                leaf, vh, uh, cw, differs = GP.pac_scl(pac, y, snr, L, snr_db2sigma)
                keep = np.ones(y.shape[0], bool)
                if random_rows:
                    keep = GP.separable(cw, y)
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
            run(torch.from_numpy(GP.GRID[rng.integers(0, GP.GRID.size, (ngrid, N))]), 1.0, False)
            run(torch.from_numpy(GP.crafted(N, rng)), 1.0, False)
            assert dropped * 100 <= total, (N, K, L, dropped, total)
            out = {k: np.concatenate(v).astype(np.float32) for k, v in rows.items()}
            zero = np.float32(0.0)
            out = {k: v + zero for k, v in out.items()}  # -0.0 -> +0.0
            path = os.path.join(HERE, f"widelist_pac_{N}_{K}_L{L}.npz")
            size = finish(path, L=np.int32(L), g=np.int32(g), info=info.astype(np.int64), **out)
            print(f"{os.path.basename(path)}: {out['y'].shape[0]} rows, {dropped} of {total} random rows dropped, "
                  f"{int((out['u_hat'] == 0).any(1).sum())} rows with a zero decision, {size} bytes", flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["polar", "pac"]
    if "polar" in which:
        gen_polar()
    if "pac" in which:
        gen_pac()
