"""fp32 restatement of CRC-aided SC-List decoding (npd_scl_decode_crc) in numpy / torch-CPU, for the tests.

The list is that of tests/pac_scl_ref.py (the same loop; g = 2, the identity convolution, gives Polar SC-List),
kept whole at the end: every final path's u, v, leaf LLRs and metric, in list order.  Two rules choose from it:
  * ml_choice: the first minimum of sum (polar_encode(u) - y)^2, PolarCode.scl_decode's use_CRC=False step;
  * ca_choice: the selection of polar.py:860-866 with the CRC defined in include/npd.h -- the passing path of
    smallest metric (first in list order on a tie), or, when no path passes, the path of smallest metric.
The CRC is the plain polynomial division of polar.py:738-748 (MSB first, zero initial register, no reflection, no
final XOR), stated as shift-and-xor on a c-bit register.  Symbol -1 is bit 1, +1 is bit 0; a path passes if its K
information decisions hold no 0 and leave remainder 0.  The K information slots carry the K - c message bits, then
the c CRC bits; for PAC codes the CRC covers the message before the convolution.

Also here: the host encoder (rate profile, convolution, Plotkin transform) and ca_words, which builds the tests'
received words on the host, so the words and what is expected of them need no GPU.
"""
import functools

import numpy as np
import torch

from pac_scl_ref import _f, _parity, _transform, pac_info, taps_of  # noqa: F401  (pac_info re-exported)


def crc_degree(poly):
    return int(poly).bit_length() - 1


def crc_remainder(bits, poly):
    """Register after feeding bits (B, n) MSB first: reg = reg << 1 | bit; reg ^= poly if bit c of reg is set."""
    bits = np.asarray(bits, dtype=np.int64)
    c = crc_degree(poly)
    reg = np.zeros(bits.shape[0], dtype=np.int64)
    for k in range(bits.shape[1]):
        reg = (reg << 1) | bits[:, k]
        reg ^= int(poly) * ((reg >> c) & 1)
    return reg


def crc_bits(bits, poly):
    """The c CRC bits (B, c) of message bits (B, K - c): the remainder of m(x) x^c, r_i = coefficient of x^(c-1-i)."""
    bits = np.asarray(bits, dtype=np.int64)
    c = crc_degree(poly)
    reg = crc_remainder(np.concatenate([bits, np.zeros((bits.shape[0], c), np.int64)], 1), poly)
    return (reg[:, None] >> np.arange(c - 1, -1, -1)[None, :]) & 1


def crc_passes(bits, poly):
    """1 where the K bits (B, K), read as a polynomial of degree K - 1, leave remainder 0."""
    return (crc_remainder(bits, poly) == 0).astype(np.int64)


def crc_attach(msg, poly):
    """(B, K - c) symbols -> (B, K): the message columns unchanged, then the CRC as +-1 (bit = msg < 0)."""
    msg = np.asarray(msg, dtype=np.float32)
    r = crc_bits((msg < 0).astype(np.int64), poly)
    return np.concatenate([msg, (1 - 2 * r).astype(np.float32)], 1)


def host_encode(msg, N, info, g=2):
    """x (B, N) = Plotkin transform of the convolution (g; 2 = none) of the rate-profiled message (B, K), +-1."""
    msg = np.asarray(msg, dtype=np.float32)
    info = np.asarray(info, dtype=np.int64)
    tap, smask = taps_of(g)
    vb = np.zeros((msg.shape[0], N), dtype=np.int64)
    vb[:, info] = (msg < 0).astype(np.int64)
    ub = np.zeros_like(vb)
    st = np.zeros(msg.shape[0], dtype=np.int64)
    for i in range(N):
        par = np.zeros_like(st)
        t = 0
        while (tap >> t) != 0:
            if (tap >> t) & 1:
                par ^= (st >> t) & 1
            t += 1
        ub[:, i] = vb[:, i] ^ par
        st = ((st << 1) | vb[:, i]) & smask
    return _transform(torch.from_numpy((1 - 2 * ub).astype(np.float32))).numpy()


def ca_words(N, K, info, g, poly, snr, B, seed):
    """(bits (B, K - c), msg (B, K) +-1 with the CRC attached, x (B, N), y (B, N) float32) built on the host."""
    c = crc_degree(poly)
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (B, K - c))
    msg = crc_attach((1 - 2 * bits).astype(np.float32), poly)
    x = host_encode(msg, N, info, g)
    y = (x + 10 ** (-snr / 20) * rng.standard_normal((B, N))).astype(np.float32)
    return bits, msg, x, y


def scl_list(y, snr, info, g, L):
    """The final list of pac_scl_ref's loop, whole: dict of u, v, leaf (S, B, N) and met (S, B) as torch tensors."""
    y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
    bs, N = y.shape
    n = N.bit_length() - 1
    info = np.asarray(info, dtype=np.int64)
    is_info = np.zeros(N, bool)
    is_info[info] = True
    tap, smask = taps_of(g)
    sigma = 10 ** (-float(snr) / 20)
    ch = (y * torch.tensor(np.float32(2 / sigma ** 2))).unsqueeze(0)
    S = 1
    lv = [torch.zeros(1, bs, 1 << d) for d in range(n)]
    u = torch.zeros(1, bs, N)
    v = torch.zeros(1, bs, N)
    leaf = torch.zeros(1, bs, N)
    cs = torch.zeros(1, bs, dtype=torch.int64)
    met = torch.zeros(1, bs)
    ar = torch.arange(bs)
    for i in range(N):
        if i == 0:
            d0 = n
        else:
            k = (i & -i).bit_length() - 1
            h = 1 << k
            top = ch.expand(S, bs, N) if k + 1 == n else lv[k + 1]
            beta = _transform(u[:, :, i - h:i])
            lv[k] = beta * top[..., :h] + top[..., h:]
            d0 = k
        for d in range(d0 - 1, -1, -1):
            top = ch.expand(S, bs, N) if d + 1 == n else lv[d + 1]
            h = 1 << d
            lv[d] = _f(top[..., :h], top[..., h:])
        l = lv[0][..., 0]
        par = _parity(cs, tap)
        u0 = (1 - 2 * par).float()
        if not is_info[i]:
            pen = l.abs() * (torch.sign(l) != u0).float()
            met = met + pen
            u[:, :, i] = u0
            v[:, :, i] = 1.0
            leaf[:, :, i] = l
            cs = (cs << 1) & smask
            continue
        s = torch.sign(l)
        cu = torch.cat([s, -s], 0)
        cm = torch.cat([met, met + l.abs()], 0)
        if 2 * S > L:
            _, inds = torch.topk(-cm, L, 0)
            si, _ = torch.sort(inds, 0)
        else:
            si = torch.arange(2 * S).unsqueeze(1).expand(2 * S, bs)
        parent = si % S
        lv = [x[parent, ar] for x in lv]
        u = u[parent, ar]
        v = v[parent, ar]
        leaf = leaf[parent, ar]
        cs = cs[parent, ar]
        u0 = u0[parent, ar]
        ui = cu[si, ar]
        vi = ui * u0
        met = cm[si, ar]
        u[:, :, i] = ui
        v[:, :, i] = vi
        leaf[:, :, i] = l[parent, ar]
        adv = ((cs << 1) | (vi < 0).long()) & smask
        cs = torch.where(ui == 0, cs, adv)
        S = si.shape[0]
    return {"u": u, "v": v, "leaf": leaf, "met": met, "y": y, "info": info}


def ml_choice(lst):
    """List index (B) of the first minimum of sum (polar_encode(u) - y)^2, summed sequentially in fp32."""
    u, y = lst["u"], lst["y"]
    S, bs, N = u.shape
    cw = _transform(u)
    dist = torch.zeros(S, bs)
    for k in range(N):
        dd = cw[:, :, k] - y[:, k].unsqueeze(0)
        dist = dist + dd * dd
    best = torch.zeros(bs, dtype=torch.int64)
    bd = dist[0].clone()
    for j in range(1, S):
        lt = dist[j] < bd
        best[lt] = j
        bd = torch.where(lt, dist[j], bd)
    return best.numpy()


def list_passes(lst, poly):
    """(S, B) 1 / 0: the path's K information decisions hold no 0 and leave remainder 0."""
    vi = lst["v"][:, :, torch.from_numpy(lst["info"])].numpy()
    S, bs, K = vi.shape
    ok = crc_passes((vi < 0).astype(np.int64).reshape(S * bs, K), poly).reshape(S, bs)
    return ok * (vi != 0).all(2)


def ca_choice(lst, poly):
    """(list index (B), crc_ok (B)): the passing path of smallest metric, or the path of smallest metric when none
    passes; the first in list order on a tie (np.argmin's first occurrence)."""
    met = lst["met"].numpy()
    ok = list_passes(lst, poly)
    anyp = ok.any(0)
    key = np.where(ok.astype(bool), met, np.float32(np.inf))
    best = np.where(anyp, key.argmin(0), met.argmin(0))
    return best.astype(np.int64), anyp.astype(np.int32)


def pick(lst, best):
    """(leaf (B, N), v_hat[:, info] (B, K), u_hat (B, N)) of list entries `best`, float32 numpy, -0.0 -> +0.0."""
    ar = np.arange(len(best))
    zero = np.float32(0.0)
    out = [lst["leaf"].numpy()[best, ar], lst["v"].numpy()[best, ar][:, lst["info"]], lst["u"].numpy()[best, ar]]
    return tuple(a + zero for a in out)


def ca_scl_ref(y, snr, info, g, L, poly):
    """(leaf LLRs (B, N), msg_hat (B, K), u_hat (B, N), crc_ok (B) int32) of the chosen path."""
    lst = scl_list(y, snr, info, g, L)
    best, ok = ca_choice(lst, poly)
    return pick(lst, best) + (ok,)


# ---------------------------------------------------------------------------------------------- the tests' word sets
#          N    K    g   poly      L   dB     classes required (a: chosen != min-metric path, b: none passes)
POLAR_SETS = [(8, 4, 2, 0xB, 4, 0.0, "abc"),
              (16, 8, 2, 0xB, 2, 0.0, "abc"),
              (32, 16, 2, 0x1D5, 1, 1.0, "bc"),
              (32, 16, 2, 0x1D5, 3, 1.0, "abc"),
              (32, 16, 2, 0x1D5, 8, 1.0, "abc"),
              (64, 32, 2, 0x61, 5, 1.0, "abc"),
              (64, 32, 2, 0x1D5, 8, 1.0, "abc"),
              (64, 32, 2, 0x11021, 4, 1.0, "abc"),
              (128, 64, 2, 0x11021, 4, 3.0, "abc"),
              (256, 128, 2, 0x1B2B117, 4, 3.0, "abc"),
              (256, 200, 2, 0xE21, 2, 5.0, "abc"),
              (16, 8, 2, 0xB, 12, 0.0, "ac"),
              (32, 16, 2, 0x1D5, 17, 1.0, "abc"),
              (64, 32, 2, 0x1D5, 32, 1.0, "abc"),
              (128, 64, 2, 0x11021, 16, 2.5, "abc"),
              (256, 128, 2, 0xE21, 32, 2.5, "abc")]
PAC_SETS = [(16, 8, 13, 0xB, 12, 0.0, "ac"),
            (32, 16, 53, 0x1D5, 4, 0.0, "abc"),
            (64, 32, 91, 0x1D5, 1, 1.0, "bc"),
            (64, 22, 91, 0x61, 8, -2.0, "abc"),
            (64, 32, 91, 0x1D5, 8, 1.0, "abc"),
            (64, 32, 91, 0x1D5, 16, 1.0, "abc"),
            (128, 64, 91, 0x11021, 4, 2.0, "bc"),
            (256, 128, 91, 0xE21, 4, 2.0, "bc"),
            (128, 64, 91, 0x11021, 32, 1.0, "abc")]
#              N    K    g   poly    L   dB   (quantised: y -> round(2y)/2, seed N + L, 200 words)
QUANT_SETS = [(32, 16, 2, 0x1D5, 8, 1.0),
              (64, 32, 91, 0x1D5, 2, 2.0),
              (128, 64, 2, 0x11021, 4, 3.0),
              (16, 8, 2, 0xB, 16, 0.0),
              (32, 16, 53, 0x1D5, 4, 0.0)]
TABLE_SETS = [s[:6] + (False,) for s in POLAR_SETS + PAC_SETS]
ALL_SETS = TABLE_SETS + [s + (True,) for s in QUANT_SETS]


def set_id(s):
    N, K, g, poly, L, snr, quant = s
    return f"{'polar' if g == 2 else 'pac'}_{N}_{K}_{poly:x}_L{L}{'_q' if quant else ''}"


def info_of(N, K, g):
    """Polar (g = 2): the reference's default information set, PolarCode(n, K) with no reliability sequence given
    (polar.py:66-110: the K highest positions); PAC: the RM rate profile."""
    if g == 2:
        from neural_polar_decoder_amd import PolarCode
        return np.asarray(PolarCode(N.bit_length() - 1, K).info_positions, dtype=np.int64)
    return pac_info(N, K)


@functools.lru_cache(maxsize=None)
def case(s):
    """One word set, decoded once per session: the words, the whole final list and what the decoder must return."""
    N, K, g, poly, L, snr, quant = s
    info = info_of(N, K, g)
    if quant:
        bits, msg, x, y = ca_words(N, K, info, g, poly, snr, 200, N + L)
        y = (np.round(2 * y) / 2).astype(np.float32)
    else:
        bits, msg, x, y = ca_words(N, K, info, g, poly, snr, 333 if N <= 64 else 77, N * 100 + K + L)
    lst = scl_list(y, snr, info, g, L)
    best, ok = ca_choice(lst, poly)
    leaf, hat, uh = pick(lst, best)
    return {"N": N, "K": K, "g": g, "poly": poly, "L": L, "snr": snr, "c": crc_degree(poly), "info": info,
            "bits": bits, "msg": msg, "x": x, "y": y, "lst": lst, "best": best, "ok": ok, "leaf": leaf, "hat": hat,
            "uh": uh}
