"""GPU: CRC-aided SC-List decoding (npd_scl_decode_crc, npd_scl_decode_crc_mc, npd_mc_generate_crc, npd_crc_attach;
PolarCode / PAC .scl_decode_crc, .scl_decode(use_CRC=True), CASCLMonteCarlo) against the fp32 restatement
tests/ca_scl_ref.py on the word sets that tests/test_ca_scl.py qualifies on the host.

Bar: bit-exact msg_hat, u_hat, crc_ok and chosen-path leaf LLRs; exact counters."""
import numpy as np
import pytest
import torch

from ca_scl_ref import ALL_SETS, TABLE_SETS, case, crc_attach, crc_degree, host_encode, set_id
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"

POLYS = {3: 0xB, 8: 0x1D5, 16: 0x11021, 6: 0x61, 11: 0xE21, 24: 0x1B2B117}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_code(N, K, g, poly=None):
    from neural_polar_decoder_amd import PAC, PolarCode
    code = PolarCode(N.bit_length() - 1, K) if g == 2 else PAC(None, N, K, g)
    if poly is not None:
        code.set_crc(crc_degree(poly), poly)
    return code


def info_of(code):
    return np.asarray(code.info_positions if hasattr(code, "info_positions") else code.B, dtype=np.int64)


def expected_leaf(cs):
    """The restatement's chosen-path leaves as the genie pass returns them: Polar adds the frozen prior (polar.py:816)."""
    leaf = cs["leaf"].copy()
    if cs["g"] == 2:
        fr = np.ones(cs["N"], bool)
        fr[cs["info"]] = False
        leaf[:, fr] = leaf[:, fr] + np.float32(1000.0)
    return leaf


@pytest.mark.parametrize("s", ALL_SETS, ids=set_id)
def test_decode_matches_the_restatement(s):
    cs = case(s)
    code = make_code(cs["N"], cs["K"], cs["g"], cs["poly"])
    assert np.array_equal(info_of(code), cs["info"])
    leaf, hat, uh, ok = code.scl_decode_crc(t(cs["y"]), cs["snr"], cs["L"], return_all=True)
    hat, uh, ok = hat.cpu().numpy(), uh.cpu().numpy(), ok.cpu().numpy()
    assert np.array_equal(ok, cs["ok"])
    assert np.array_equal(hat, cs["hat"])
    assert np.array_equal(uh, cs["uh"])
    assert np.array_equal(leaf.cpu().numpy(), expected_leaf(cs))
    # where a path passed, re-attaching the decoded message reproduces the decoded CRC columns
    kc = cs["K"] - cs["c"]
    good = ok == 1
    assert good.any()
    again = code.crc_attach(t(hat[good][:, :kc])).cpu().numpy()
    assert np.array_equal(again, hat[good])
    # the public return: (leaf, msg_hat[:, :K - c]) and crc_ok on request; outputs are optional one by one
    l2, m2, o2 = code.scl_decode_crc(t(cs["y"]), cs["snr"], cs["L"], want_llrs=False, return_ok=True)
    assert l2 is None and np.array_equal(m2.cpu().numpy(), cs["hat"][:, :kc]) and np.array_equal(o2.cpu().numpy(), ok)


@pytest.mark.parametrize("K,c", [(4, 3), (16, 8), (32, 16), (140, 16), (200, 11), (256, 24)])
def test_crc_attach_matches_the_restatement(K, c):
    from neural_polar_decoder_amd import _lib
    rng = np.random.default_rng(K * 100 + c)
    m = (1.0 - 2.0 * rng.integers(0, 2, (70, K - c))).astype(np.float32)
    m[3] *= np.float32(0.25)   # any negative value is bit 1; the message columns are copied unchanged
    m[4, 0] = 0.0              # 0 is bit 0
    msg = t(m)
    out = torch.full((70, K), 7.0, device=DEV)
    _lib.check(_lib.load().npd_crc_attach(_lib.ptr(msg), _lib.ptr(out), 70, K, POLYS[c], _lib.stream_of(msg.device)),
               "npd_crc_attach")
    assert np.array_equal(out.cpu().numpy(), crc_attach(m, POLYS[c]))


GEN_SHAPES = [(64, 32, 2, 8), (128, 64, 91, 16), (256, 200, 2, 24), (256, 140, 2, 16)]


@pytest.mark.parametrize("N,K,g,c", GEN_SHAPES)
def test_mc_generate_crc(N, K, g, c):
    code = make_code(N, K, g, POLYS[c])
    B, snr, seed, si, off = 700, 2.0, 77, 3, 12345
    msg, x, y = code.mc_generate_crc(B, snr, seed, si, off, device=DEV, want_x=True)
    m0, x0, y0 = code.mc_generate(B, snr, seed, si, off, device=DEV, want_x=True)
    msg, m0 = msg.cpu().numpy(), m0.cpu().numpy()
    assert msg.shape == (B, K) and np.array_equal(msg[:, :K - c], m0[:, :K - c])
    assert np.array_equal(msg, crc_attach(m0[:, :K - c], POLYS[c]))
    assert not np.array_equal(msg, m0), "the CRC columns replace Philox bits"
    assert np.array_equal(x.cpu().numpy(), host_encode(msg, N, info_of(code), g))
    # the noise is the channel's for the same (seed, SNR index, codeword index): y = x + fl32(sigma z), as npd_awgn
    code.manual_seed(seed)
    code._rng.take(off)
    assert torch.equal(y, code.channel(x, snr, snr_index=si))
    code.manual_seed(seed)
    code._rng.take(off)
    assert torch.equal(y0, code.channel(x0, snr, snr_index=si))
    # msg and x are optional, and an output buffer is honoured
    buf = torch.empty(B, N, device=DEV)
    m2, x2, y2 = code.mc_generate_crc(B, snr, seed, si, off, want_msg=False, out=buf)
    assert m2 is None and x2 is None and y2 is buf and torch.equal(buf, y)


COUNT_SHAPES = [(32, 16, 2, 8, 4, 3000, 1.0), (128, 64, 91, 16, 8, 1000, 2.0), (256, 200, 2, 24, 2, 1000, 5.0),
                (256, 140, 2, 16, 12, 500, 3.0)]


@pytest.mark.parametrize("N,K,g,c,L,B,snr", COUNT_SHAPES)
def test_fused_counters_are_exact(N, K, g, c, L, B, snr):
    code = make_code(N, K, g, POLYS[c])
    seed, off = 5, 999
    msg, _, y = code.mc_generate_crc(B, snr, seed, 0, off, device=DEV)
    _, hat, _, ok = code.scl_decode_crc(y, snr, L, want_llrs=False, return_all=True)
    cnt = torch.full((3,), 10, dtype=torch.int64, device=DEV)
    hat2 = torch.empty(B, K, device=DEV)
    code.scl_decode_crc_mc(y, snr, L, seed, off, cnt, msg_hat=hat2)
    assert torch.equal(hat, hat2)
    wrong = (msg[:, :K - c] != hat[:, :K - c]).cpu().numpy()
    want = [10 + int(wrong.sum()), 10 + int(wrong.any(1).sum()), 10 + int((ok == 0).sum())]
    print((N, K, g, c, L), "bit / block / crc_fail:", [w - 10 for w in want])
    assert cnt.cpu().tolist() == want
    assert want[1] > 10 and want[2] > 10, "the shape exercises both counters"
    # without msg_hat
    cnt2 = torch.zeros(3, dtype=torch.int64, device=DEV)
    code.scl_decode_crc_mc(y, snr, L, seed, off, cnt2)
    assert cnt2.cpu().tolist() == [w - 10 for w in want]


@pytest.mark.parametrize("family", ["polar", "pac"])
def test_noiseless_words_decode_exactly(family):
    shapes = sorted({s[:5] for s in TABLE_SETS if (s[2] == 2) == (family == "polar")})
    assert len(shapes) == (16 if family == "polar" else 9)
    for N, K, g, poly, L in shapes:
        code = make_code(N, K, g, poly)
        c = crc_degree(poly)
        rng = np.random.default_rng(N + K + L)
        m = (1.0 - 2.0 * rng.integers(0, 2, (65, K - c))).astype(np.float32)
        x = code.encode_with_crc(t(m), c) if poly == POLYS[c] else code.encode(code.crc_attach(t(m)))
        assert np.array_equal(x.cpu().numpy(), host_encode(crc_attach(m, poly), N, info_of(code), g))
        _, hat, ok = code.scl_decode_crc(x, 2.0, L, want_llrs=False, return_ok=True)
        assert np.array_equal(hat.cpu().numpy(), m), (N, K, g, L)
        assert bool((ok == 1).all()), (N, K, g, L)


def test_monte_carlo_shards_sum_to_the_single_run():
    from neural_polar_decoder_amd.montecarlo import CASCLMonteCarlo
    for g in (2, 91):
        code = make_code(64, 32, g, POLYS[8])
        snrs = [1.0, 2.0]
        one = CASCLMonteCarlo(code, 4, snrs, 3000, 512, seed=9)
        r1 = one.run()
        assert r1.K == 24 and r1.codewords == 3000 and one.crc_len == 8
        parts = []
        for rank in range(3):
            d = CASCLMonteCarlo(code, 4, snrs, 3000, 512, seed=9, rank=rank, world=3)
            parts.append((d.run(), d.crc_fail))
        for si in range(2):
            assert sum(p.bit_errors[si] for p, _ in parts) == r1.bit_errors[si]
            assert sum(p.block_errors[si] for p, _ in parts) == r1.block_errors[si] > 0
            assert sum(f[si] for _, f in parts) == one.crc_fail[si] > 0
    with pytest.raises(ValueError):
        CASCLMonteCarlo(make_code(64, 32, 2), 4, [1.0], 10, 10)


def test_empty_batch():
    for g in (2, 53):
        code = make_code(32, 16, g, POLYS[8])
        leaf, hat, uh, ok = code.scl_decode_crc(torch.empty(0, 32, device=DEV), 1.0, 4, return_all=True)
        assert leaf.shape == (0, 32) and hat.shape == (0, 16) and uh.shape == (0, 32) and ok.shape == (0,)
        cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
        code.scl_decode_crc_mc(torch.empty(0, 32, device=DEV), 1.0, 4, 1, 0, cnt)
        assert cnt.cpu().tolist() == [0, 0, 0]
        msg, _, y = code.mc_generate_crc(0, 1.0, 1, device=DEV)
        assert msg.shape == (0, 16) and y.shape == (0, 32)
        assert code.crc_attach(torch.empty(0, 8, device=DEV)).shape == (0, 16)


def test_scl_decode_use_crc_is_scl_decode_crc():
    for g in (2, 53):
        code = make_code(32, 16, g)
        rng = np.random.default_rng(g)
        m = t((1.0 - 2.0 * rng.integers(0, 2, (200, 8))).astype(np.float32))
        x = code.encode_with_crc(m, 8)
        assert (code.CRC_len, code.K_minus_CRC, code.crc_poly) == (8, 8, 0x1D5)
        code.manual_seed(4)
        y = code.channel(x, 1.0)
        leaf, hat = code.scl_decode(y, 1.0, 4, use_CRC=True)
        l2, h2, ok = code.scl_decode_crc(y, 1.0, 4, return_ok=True)
        assert hat.shape == (200, 8) and torch.equal(hat, h2) and torch.equal(leaf, l2)
        assert 0 < int(ok.sum()) and float((hat == m).all(1).float().mean()) > 0.3
        # host in -> host out, as scl_decode
        lh, hh = code.scl_decode(y.cpu(), 1.0, 4, use_CRC=True)
        assert not hh.is_cuda and torch.equal(hh, hat.cpu()) and torch.equal(lh, leaf.cpu())
        # CRC_len = 0 is the plain encoder, and use_CRC=True then has nothing to check
        assert torch.equal(code.encode_with_crc(torch.ones(3, 16, device=DEV), 0), code.encode(torch.ones(3, 16, device=DEV)))
        with pytest.raises(NotImplementedError):
            code.scl_decode(y, 1.0, 4, use_CRC=True)


@pytest.mark.parametrize("name", ["scl_64_32_L8", "pac_scl_128_64_L4"])
def test_plain_scl_is_unchanged_after_a_crc_call(name):
    d = golden(f"{name}.npz")
    N, K = d["y"].shape[1], len(d["info"])
    if "g" in d.files:
        code = make_code(N, K, int(d["g"]))
    else:  # the fixture's own information set (the reference's 'polar' reliability order)
        from neural_polar_decoder_amd import PolarCode
        code = PolarCode(N.bit_length() - 1, K, F=np.setdiff1d(np.arange(N), d["info"]))
    assert np.array_equal(info_of(code), d["info"])
    for s in np.unique(d["snr"]):
        m = d["snr"] == s
        y = t(d["y"][m])
        code.set_crc(8)
        code.scl_decode_crc(y, float(s), int(d["L"]))
        leaf, hat = code.scl_decode(y, float(s), int(d["L"]))
        assert np.array_equal(hat.cpu().numpy(), d["msg_hat"][m]), (name, s)
        assert np.array_equal(leaf.cpu().numpy(), d["leaf"][m]), (name, s)
        code.set_crc(0)
        _, hat0 = code.scl_decode(y, float(s), int(d["L"]), want_llrs=False)
        assert torch.equal(hat0, hat)
