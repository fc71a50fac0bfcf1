"""fp32 restatement of PAC SC-List decoding (PAC.pac_scl_decode) in numpy / torch-CPU, for the tests.

The rules: PolarCode.scl_decode (polar.py:793-876, use_CRC=False, pruneLists at 777-791) with its leaf step
replaced by pac_sc_decode's (pac_code.py:534-573).
  * LLRs fl32(y * fl32(2 / sigma^2)); min-sum f / g; no priors.
  * Every path carries its convolution state (the last len(g_array) - 1 values of v_hat, initially +1), here a
    bit mask (bit t set iff v_{i-1-t} = -1); u0 = conv1bTrans(+1, state) = (-1)^parity(state & taps).
  * Frozen position: v = +1, u = u0, the state advances with +1, the metric becomes fl32(m + |l|) unless
    sign(l) == u0 (sign(0) = 0 never is; the penalty is then 0).
  * Information position: the list forks, in list order, into [keep_0 .. keep_{s-1}, flip_0 .. flip_{s-1}];
    keep has u = sign(l), metric m; flip has u = -sign(l), metric fl32(m + |l|); v = u * u0 advances the state;
    l == 0 gives u = v = 0 and the state does not advance.  More than L children: torch.topk(-metric, L) picks
    the survivors, kept in ascending child order.
  * Final path: first minimum over the live list of sum (polar_encode(u) - y)^2, summed sequentially in fp32.
g = 2 (g_array = [-1, +1], no tap) is the identity convolution (u = v): Polar SC-List's decisions.
"""
import numpy as np
import torch


def taps_of(g):
    """(tap mask, state mask) of the polynomial g, bit t <-> state[t] = v_{i-1-t} (g_array[t + 1] == -1)."""
    M = int(g).bit_length()
    tap = 0
    for j in range(1, M):
        if (int(g) >> (M - 1 - j)) & 1:
            tap |= 1 << (j - 1)
    return tap, (1 << (M - 1)) - 1


def pac_info(N, K):
    """The RM rate profile of PAC(N, K) (pac_code.py:108-111): the K positions of largest Hamming weight."""
    w = np.array([bin(i).count("1") for i in range(N)])
    return np.sort(np.argsort(w)[-K:])


def _transform(u):
    """Plotkin transform along the last axis (length a power of two): (a, b) -> (a * b, b) at every stage."""
    x = u.clone()
    h = x.shape[-1]
    step = 1
    while step < h:
        v = x.view(*x.shape[:-1], h // (2 * step), 2, step)
        v[..., 0, :] *= v[..., 1, :]
        step *= 2
    return x


def _f(a, b):
    return torch.sign(a) * torch.sign(b) * torch.minimum(a.abs(), b.abs())


def _parity(cs, tap):
    p = torch.zeros_like(cs)
    t = 0
    while (tap >> t) != 0:
        if (tap >> t) & 1:
            p ^= (cs >> t) & 1
        t += 1
    return p


def pac_scl_ref(y, snr, info, g, L):
    """(leaf LLRs of the chosen path (B,N), v_hat[:, info] (B,K), u_hat (B,N)) as float32 numpy arrays."""
    y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
    bs, N = y.shape
    n = N.bit_length() - 1
    info = np.asarray(info, dtype=np.int64)
    is_info = np.zeros(N, bool)
    is_info[info] = True
    tap, smask = taps_of(g)
    sigma = 10 ** (-float(snr) / 20)
    ch = (y * torch.tensor(np.float32(2 / sigma ** 2))).unsqueeze(0)  # (1, bs, N): shared by the whole list
    S = 1
    lv = [torch.zeros(1, bs, 1 << d) for d in range(n)]               # level d of every path
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
        cu = torch.cat([s, -s], 0)                                    # (2S, bs) children in list order
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
    zero = np.float32(0.0)
    out = [leaf[best, ar].numpy(), v[best, ar][:, torch.from_numpy(info)].numpy(), u[best, ar].numpy()]
    return tuple(a + zero for a in out)  # -0.0 -> +0.0
