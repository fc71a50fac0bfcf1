"""Writes tests/golden/crc_ref.npz: the reference's own CRC helpers on random bit vectors.

    python tests/golden/gen_crc.py /path/to/reference

PolarCode.get_CRC and PolarCode.CRC_check (polar.py:738-763) read a module global `polar` that exists only when
polar.py runs as a script; it is injected here (`polar_module.polar = code`), with CRC_len and K_minus_CRC set as
encode_with_crc sets them (polar.py:765-767).  Only data is stored, per CRC length c in {3, 8, 16} and message length
K - c in {1, 5, 8, 24}: random message bits, get_CRC's remainder, and CRC_check of [bits, remainder] (1), of
[bits, complemented remainder] and of a word with one flipped bit (both as the reference answers them).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 24


def main(ref):
    sys.path.insert(0, ref)
    import polar as polar_module
    out = {}
    rng = np.random.default_rng(738)
    for c in (3, 8, 16):
        for kc in (1, 5, 8, 24):
            K = kc + c
            n = 5
            while (1 << n) < 2 * K:
                n += 1
            code = polar_module.PolarCode(n, K, None)
            code.CRC_len = c
            code.K_minus_CRC = kc
            polar_module.polar = code
            poly = int("".join(str(int(b)) for b in code.CRC_polynomials[c]), 2)
            bits = rng.integers(0, 2, (ROWS, kc)).astype(np.int32)
            bits[0] = 0
            bits[1] = 1
            rem = np.stack([code.get_CRC(torch.from_numpy(b.copy()).int()).numpy() for b in bits]).astype(np.int32)
            words = np.concatenate([bits, rem], 1)
            comp = np.concatenate([bits, 1 - rem], 1)
            flip = words.copy()
            flip[np.arange(ROWS), rng.integers(0, K, ROWS)] ^= 1

            def chk(w):
                return np.array([code.CRC_check(torch.from_numpy(r.copy()).int()) for r in w], np.int32)

            key = f"c{c}_k{kc}"
            out[key + "_poly"] = np.int64(poly)
            out[key + "_bits"] = bits
            out[key + "_rem"] = rem
            out[key + "_flip"] = flip
            out[key + "_check"] = chk(words)
            out[key + "_check_comp"] = chk(comp)
            out[key + "_check_flip"] = chk(flip)
    np.savez_compressed(os.path.join(HERE, "crc_ref.npz"), **out)
    print("crc_ref.npz:", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
