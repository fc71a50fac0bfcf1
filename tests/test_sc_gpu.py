"""GPU parity: encoder, channel, SC / PAC-SC decoders and counters through the C-ABI
(neural_polar_decoder_amd -> libnpd.so) against the reference's golden vectors and the oracle."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

SC_CASES = [(32, 16), (64, 32), (128, 64), (256, 128), (16, 8), (64, 22)]
PAC_CASES = [(128, 64), (64, 22), (32, 16)]
DEV = "cuda:0"


def polar_for(N, info):
    from neural_polar_decoder_amd import PolarCode
    n = int(np.log2(N))
    K = len(info)
    F = np.array(sorted(set(range(N)) - set(int(i) for i in info)))
    return PolarCode(n, K, F=F)


def pac_for(N, K):
    import argparse
    from neural_polar_decoder_amd import PAC
    return PAC(argparse.Namespace(target_K=K), N, K, 91)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_encode_plotkin_golden():
    e = golden("encode.npz")
    for N, K in [(32, 16), (64, 32), (128, 64), (256, 128), (8, 4)]:
        code = polar_for(N, e[f"info_{N}_{K}"])
        x = code.encode_plotkin(t(e[f"msg_{N}_{K}"])).cpu().numpy()
        assert np.array_equal(x, e[f"x_{N}_{K}"]), N
    code = polar_for(16, e["info_16_8"])
    assert np.array_equal(code.encode_plotkin(t(e["msgf_16_8"])).cpu().numpy(), e["xf_16_8"])


def test_pac_encode_golden():
    e = golden("encode.npz")
    for N, K in PAC_CASES:
        pac = pac_for(N, K)
        assert np.array_equal(pac.B, e[f"pinfo_{N}_{K}"])
        x = pac.pac_encode(t(e[f"pmsg_{N}_{K}"]), scheme="RM").cpu().numpy()
        assert np.array_equal(x, e[f"px_{N}_{K}"]), N


@pytest.mark.parametrize("N,K", SC_CASES)
def test_sc_decode_golden(N, K):
    d = golden(f"sc_polar_{N}_{K}.npz")
    code = polar_for(N, d["info"])
    for s in np.unique(d["snr"]):
        m = d["snr"] == s
        leaf, hat = code.sc_decode_new(t(d["y"][m]), float(s))
        assert np.array_equal(leaf.cpu().numpy(), d["leaf"][m]), (N, s)
        assert np.array_equal(hat.cpu().numpy(), d["msg_hat"][m]), (N, s)
        hat2 = code.sc_decode_msg(t(d["y"][m]), float(s))  # fast (msg-only) kernel variant
        assert np.array_equal(hat2.cpu().numpy(), d["msg_hat"][m]), (N, s)
    gl, gh = code.sc_decode_new(t(d["gt_y"]), float(d["gt_snr"]), use_gt=t(d["gt"]))
    assert np.array_equal(gl.cpu().numpy(), d["gt_leaf"]) and np.array_equal(gh.cpu().numpy(), d["gt_msg_hat"])


@pytest.mark.parametrize("N,K", PAC_CASES)
def test_pac_sc_decode_golden(N, K):
    d = golden(f"sc_pac_{N}_{K}.npz")
    pac = pac_for(N, K)
    for s in np.unique(d["snr"]):
        m = d["snr"] == s
        leaf, hat, uh = pac.pac_sc_decode(t(d["y"][m]), float(s))
        assert np.array_equal(leaf.cpu().numpy(), d["leaf"][m])
        assert np.array_equal(hat.cpu().numpy(), d["msg_hat"][m])
        assert np.array_equal(uh.cpu().numpy(), d["u_hat"][m])
    gl, gh, gu = pac.pac_sc_decode(t(d["gt_y"]), float(d["gt_snr"]), use_gt_codeword=t(d["gt"]))
    assert np.array_equal(gl.cpu().numpy(), d["gt_leaf"])
    assert np.array_equal(gh.cpu().numpy(), d["gt_msg_hat"])
    assert np.array_equal(gu.cpu().numpy(), d["gt_u_hat"])


@pytest.mark.parametrize("N,K", [(4, 2), (8, 4), (16, 8), (32, 16), (64, 32), (128, 64), (256, 128), (64, 1), (64, 64)])
def test_sc_decode_vs_oracle_random(oracle, N, K):
    """Ragged batch sizes (tails of the 64-codeword tiles), all code lengths, edge rates."""
    from neural_polar_decoder_amd.codes import polar_info_positions
    info = polar_info_positions(N, K)
    code = polar_for(N, info)
    rng = np.random.default_rng(N * 131 + K)
    for B in (1, 63, 65, 1000):
        y = (rng.standard_normal((B, N)) + (1 - 2 * (rng.random((B, N)) < 0.5))).astype(np.float32)
        leaf, hat = code.sc_decode_new(t(y), 1.5)
        ol, oh = oracle.sc_decode(y, 1.5, info)
        assert np.array_equal(leaf.cpu().numpy(), ol) and np.array_equal(hat.cpu().numpy(), oh), B


def _case(defaults, *vals, **more):
    """pytest.param of vals plus the parameters added later (defaults, overridden by more).  The id is the one the
    case had before those parameters existed, with the overrides appended: adding a parameter renames no case."""
    extra = {**defaults, **more}
    return pytest.param(*vals, *extra.values(), id="-".join([str(v) for v in vals] + [f"{k}{v}" for k, v in more.items()]))


# B = 130: two full 64-word tiles and a 2-row tail (tile loop, tail clamp, uncounted tail lanes)
@pytest.mark.parametrize("N,K,B", [(128, 64, 777), (4, 2, 130), (8, 4, 130), (16, 8, 130), (256, 128, 130)])
def test_pac_vs_oracle_random(oracle, N, K, B):
    """The PAC kernels with leaf LLR / u_hat outputs, and with genie decisions, at every length no golden file has."""
    pac = pac_for(N, K)
    rng = np.random.default_rng(3)
    y = rng.standard_normal((B, N)).astype(np.float32)
    leaf, hat, uh = pac.pac_sc_decode(t(y), 0.5)
    ol, oh, ou = oracle.pac_sc_decode(y, 0.5, pac.B)
    assert np.array_equal(leaf.cpu().numpy(), ol)
    assert np.array_equal(hat.cpu().numpy(), oh)
    assert np.array_equal(uh.cpu().numpy(), ou)
    gt = (1 - 2 * (rng.random((B, N)) < 0.5)).astype(np.float32)
    leaf, hat, uh = pac.pac_sc_decode(t(y), 0.5, use_gt_codeword=t(gt))
    ol, oh, ou = oracle.pac_sc_decode(y, 0.5, pac.B, gt=gt)
    assert np.array_equal(leaf.cpu().numpy(), ol)
    assert np.array_equal(hat.cpu().numpy(), oh)
    assert np.array_equal(uh.cpu().numpy(), ou)


def test_channel_statistics():
    from neural_polar_decoder_amd import reference_polar_code
    code = reference_polar_code(64, 32)
    code.manual_seed(7)
    x = torch.ones(1 << 16, 64, device=DEV)
    for snr in (0.0, 3.0):
        y = code.channel(x, snr)
        n = (y - x).double()
        sigma = 10 ** (-snr / 20)
        assert abs(n.mean().item()) < 5e-3 * sigma
        assert abs(n.std().item() / sigma - 1) < 5e-3
    y1, y2 = code.channel(x, 1.0), code.channel(x, 1.0)
    assert not torch.equal(y1, y2)  # the counter advances between calls


def test_awgn_matches_oracle(oracle):
    rng = np.random.default_rng(9)
    x = (1 - 2 * (rng.random((333, 64)) < 0.5)).astype(np.float32)
    from neural_polar_decoder_amd import _lib
    from neural_polar_decoder_amd.utils import sigma_f32
    xd = t(x)
    y = torch.empty_like(xd)
    _lib.check(_lib.load().npd_awgn(_lib.ptr(xd), _lib.ptr(y), 333, 64, sigma_f32(2.0), 99, 3, 1000,
                                    _lib.stream_of(xd.device)))
    yo = oracle.awgn(x, 2.0, 99, 3, 1000)
    assert np.abs(y.cpu().numpy() - yo).max() < 2e-5


@pytest.mark.parametrize("N,K,pac", [(64, 32, False), (32, 16, False), (256, 128, False), (128, 64, True)])
def test_mc_generate_matches_oracle(oracle, N, K, pac):
    if pac:
        code = pac_for(N, K)
        info = code.B
    else:
        from neural_polar_decoder_amd import reference_polar_code
        code = reference_polar_code(N, K)
        info = code.info_positions
    msg, x, y = code.mc_generate(2000, 1.0, seed=1234, snr_index=2, cw_offset=777, want_msg=True, want_x=True)
    om = oracle.gen_msg(2000, K, 1234, 777)
    assert np.array_equal(msg.cpu().numpy(), om)
    ox = oracle.pac_encode(om, N, info) if pac else oracle.encode_plotkin(om, N, info)
    assert np.array_equal(x.cpu().numpy(), ox)
    oy = oracle.awgn(ox, 1.0, 1234, 2, 777)
    assert np.abs(y.cpu().numpy() - oy).max() < 2e-5


_MC = dict(B=5000, generic=False)


@pytest.mark.parametrize("N,K,pac,B,generic", [
    _case(_MC, 64, 32, False), _case(_MC, 32, 16, False), _case(_MC, 128, 64, False), _case(_MC, 256, 128, False),
    _case(_MC, 128, 64, True), _case(_MC, 64, 22, True),
    _case(_MC, 4, 2, True, B=130), _case(_MC, 8, 4, True, B=130), _case(_MC, 16, 8, True, B=130),
    _case(_MC, 256, 128, True, B=130), _case(_MC, 4, 2, False, B=130), _case(_MC, 8, 4, False, B=130, generic=True),
    _case(_MC, 16, 8, False, B=130, generic=True)])
def test_sc_decode_mc_counters_exact(oracle, monkeypatch, N, K, pac, B, generic):
    """Fused decode+count on GPU-generated y == oracle decode + count on the same y (bit-exact).  The B = 130
    cases reach the msg-only kernels no other case does: PAC at N = 4, 8, 16, 256, and (generic: NPD_SC_GENERIC=1,
    read per call) the generic Polar kernel at the lengths the fast kernel otherwise takes."""
    if pac:
        code = pac_for(N, K)
        info = code.B
    else:
        from neural_polar_decoder_amd import reference_polar_code
        code = reference_polar_code(N, K)
        info = code.info_positions
    if generic:
        monkeypatch.setenv("NPD_SC_GENERIC", "1")
    seed, off = 42, 12345
    for si, snr in enumerate([0.0, 2.0, 4.0]):
        msg, _, y = code.mc_generate(B, snr, seed, si, off)
        cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
        hat = torch.empty(B, K, device=DEV)
        code.sc_decode_mc(y, snr, seed, off, cnt, msg_hat=hat)
        yh = y.cpu().numpy()
        if pac:
            _, oh, _ = oracle.pac_sc_decode(yh, snr, info)
        else:
            _, oh = oracle.sc_decode(yh, snr, info)
        assert np.array_equal(hat.cpu().numpy(), oh)
        be, bl = oracle.count_errors(msg.cpu().numpy(), oh)
        assert cnt.cpu().tolist() == [be, bl], (snr, cnt.cpu().tolist(), be, bl)


def test_pac_static_frozen_set_kernel(monkeypatch, oracle):
    """PAC(128,64) 'RM' msg-only decoding runs the kernel with the frozen set compiled in (rate-0 subtrees
    decoded without LLRs); NPD_SC_NOSPEC=1 forces the run-time frozen set.  Identical msg_hat and counts, and
    equal to the oracle, on noisy words plus crafted rows (zeros, huge and tiny magnitudes, constants)."""
    code = pac_for(128, 64)
    msg, _, y = code.mc_generate(3000 + 11, 1.0, 77, 0, 0)
    rng = np.random.default_rng(3)
    crafted = np.stack([np.zeros(128), np.full(128, 1e30), -np.full(128, 1e-30), rng.standard_normal(128) * 1e6,
                        np.where(rng.random(128) < 0.5, 0.0, 1.0), np.full(128, -1.0)]).astype(np.float32)
    y[: crafted.shape[0]] = torch.from_numpy(crafted).to(DEV)
    out = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("NPD_SC_NOSPEC", env)
        cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
        hat = torch.empty(y.shape[0], 64, device=DEV)
        code.sc_decode_mc(y, 1.0, 77, 0, cnt, msg_hat=hat)
        out.append((hat.cpu().numpy(), cnt.cpu().tolist()))
    monkeypatch.delenv("NPD_SC_NOSPEC")
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    _, oh, _ = oracle.pac_sc_decode(y.cpu().numpy(), 1.0, code.B)
    assert np.array_equal(out[0][0], oh)


def test_count_errors_golden():
    from neural_polar_decoder_amd import errors_ber, errors_bler
    d = golden("errors.npz")
    assert float(errors_ber(t(d["ref"]), t(d["hat"]))) == pytest.approx(float(d["ber"]), abs=0)
    assert errors_bler(t(d["ref"]), t(d["hat"])) == pytest.approx(float(d["bler"]), abs=0)


def test_full_size_properties():
    """B = 2^20 (config C2): noiseless round trip, shard invariance, counters == separate count."""
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.utils import count_errors
    code = reference_polar_code(64, 32)
    B = 1 << 20
    msg, x, y = code.mc_generate(B, 2.0, seed=5, snr_index=0, cw_offset=0, want_x=True)
    # noiseless: decoding the clean codeword returns the message exactly (every bit, every codeword)
    hat = code.sc_decode_msg(x, 2.0)
    assert torch.equal(hat, msg)
    # decode + fused count == decode then separate count
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    hat = torch.empty(B, 32, device=DEV)
    code.sc_decode_mc(y, 2.0, 5, 0, cnt, msg_hat=hat)
    assert torch.equal(hat, code.sc_decode_msg(y, 2.0))
    c2 = count_errors(msg, hat)
    assert torch.equal(cnt, c2)
    # sharding invariance: two half launches with offsets == one launch
    c3 = torch.zeros(2, dtype=torch.int64, device=DEV)
    code.sc_decode_mc(y[: B // 2], 2.0, 5, 0, c3)
    code.sc_decode_mc(y[B // 2:], 2.0, 5, B // 2, c3)
    assert torch.equal(cnt, c3)


def test_ber_curve_matches_reference_anchors():
    """SC BLER/BER at 2^22 codewords per SNR (fused Monte-Carlo, Philox words) vs the reference's own
    sc_decode_new curve (tests/golden/sc_anchors_64_32.npz: 2e5 words at 0-1 dB, 1e6 at 2-4 dB, torch RNG):
    within 4 two-sample standard errors (BLER binomial; BER with block-clustered bit errors bounded by the
    block-level variance), and the BLER curve's horizontal offset from the reference's within +-0.05 dB at every
    point (the north_star's BER-curve bar; standard error of the offset ~0.004-0.01 dB here)."""
    from conftest import db_offsets
    from neural_polar_decoder_amd import reference_polar_code
    ref = golden("sc_anchors_64_32.npz")
    snrs = [float(s) for s in ref["snr"]]
    code = reference_polar_code(64, 32)
    B = 1 << 22
    cnt = torch.zeros(len(snrs), 2, dtype=torch.int64, device=DEV)
    for off in range(0, B, 1 << 20):
        code.sc_mc_sweep_fused(1 << 20, snrs, 1234, off, cnt)
    c = cnt.cpu().numpy()
    bler = []
    for si, s in enumerate(snrs):
        nr = int(ref["n"][si])
        p, pr = c[si, 1] / B, int(ref["blk_err"][si]) / nr
        ber, ber_r = c[si, 0] / (B * 32), int(ref["bit_err"][si]) / (nr * 32)
        se = np.sqrt(pr * (1 - pr) * (1 / nr + 1 / B))
        assert abs(p - pr) < 4 * se + 1e-12, (s, p, pr)
        # bit errors per erroneous block <= K: Var(errors per word) <= K * E[errors per word]
        se_ber = np.sqrt(32 * ber_r * 32 * (1 / nr + 1 / B)) / 32
        assert abs(ber - ber_r) < 4 * se_ber + 1e-12, (s, ber, ber_r)
        bler.append(p)
    offs = db_offsets(snrs, bler, snrs, [int(x) / int(n) for x, n in zip(ref["blk_err"], ref["n"])])
    for s, o in zip(snrs, offs):
        assert o is not None and abs(o) <= 0.05, (s, o)


def test_montecarlo_driver_shard_invariance():
    """SCMonteCarlo: simulated 3-rank shards (summed) == one rank, exactly (Philox keyed by codeword)."""
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.montecarlo import SCMonteCarlo
    code = reference_polar_code(64, 32)
    snrs = [0.0, 1.0, 2.0]
    one = SCMonteCarlo(code, snrs, 100_003, 40_000, seed=7, rank=0, world=1).run()
    parts = [SCMonteCarlo(code, snrs, 100_003, 40_000, seed=7, rank=r, world=3).run() for r in range(3)]
    assert [sum(p.bit_errors[i] for p in parts) for i in range(3)] == one.bit_errors
    assert [sum(p.block_errors[i] for p in parts) for i in range(3)] == one.block_errors


def test_montecarlo_pac_and_gru_drivers_run():
    import argparse
    from neural_polar_decoder_amd import PAC, reference_polar_code
    from neural_polar_decoder_amd.montecarlo import GRUMonteCarlo, SCMonteCarlo
    from neural_polar_decoder_amd.rnn import RNN_Model, RNN_decoder
    pac = PAC(argparse.Namespace(target_K=64), 128, 64, 91)
    r = SCMonteCarlo(pac, [2.0], 20_000, 8192).run()
    assert 0 < r.ber[0] < 0.2
    code = reference_polar_code(64, 32)
    torch.manual_seed(0)
    net = RNN_Model("GRU", 66, 64, 1, 2, 64, 0, 0).to(DEV)
    dec = RNN_decoder("y_input", 64, code.info_positions, onehot=True)
    g = GRUMonteCarlo(code, net, dec, [0.0, 4.0], 2048, 1024).run()
    assert all(0.3 < b < 0.7 for b in g.ber)  # untrained weights: coin flips


@pytest.mark.parametrize("N,K", [(64, 32), (32, 16), (16, 8), (64, 22)])
def test_msg_only_fast_paths_on_golden_including_crafted_rows(N, K):
    """msg-only decoding takes the streaming kernels (for these standard codes the frozen-set-specialised
    one, whose closed-form subtrees fall back to step-by-step SC on huge or zero LLRs): same msg_hat as
    the reference on every golden row, including the crafted zero / |LLR| >> 1000 rows."""
    d = golden(f"sc_polar_{N}_{K}.npz")
    code = polar_for(N, d["info"])
    for s in np.unique(d["snr"]):
        m = d["snr"] == s
        y = t(d["y"][m])
        assert np.array_equal(code.sc_decode_msg(y, float(s)).cpu().numpy(), d["msg_hat"][m]), (N, s)
        cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
        hat = torch.empty(y.shape[0], K, device=DEV)
        code.sc_decode_mc(y, float(s), 1, 0, cnt, msg_hat=hat)
        assert np.array_equal(hat.cpu().numpy(), d["msg_hat"][m]), (N, s)


def test_specialised_8_4_and_high_snr_vs_oracle(oracle):
    from neural_polar_decoder_amd import reference_polar_code
    for N, K in [(8, 4), (64, 32), (32, 16)]:
        code = reference_polar_code(N, K)
        for snr in (-2.0, 6.0, 12.0):
            _, _, y = code.mc_generate(20000, snr, seed=4, want_msg=False)
            _, oh = oracle.sc_decode(y.cpu().numpy(), snr, code.info_positions)
            assert np.array_equal(code.sc_decode_msg(y, snr).cpu().numpy(), oh), (N, snr)


_FUSED = dict(generic=False)


@pytest.mark.parametrize("N,K,B,generic", [
    _case(_FUSED, 64, 32, 100_003), _case(_FUSED, 32, 16, 5000), _case(_FUSED, 16, 8, 777), _case(_FUSED, 64, 22, 3001),
    _case(_FUSED, 8, 4, 4099), _case(_FUSED, 4, 2, 1000), _case(_FUSED, 128, 64, 20_001), _case(_FUSED, 256, 128, 3333),
    _case(_FUSED, 256, 200, 700), _case(_FUSED, 8, 4, 130, generic=True), _case(_FUSED, 16, 8, 130, generic=True),
    _case(_FUSED, 32, 16, 130, generic=True), _case(_FUSED, 64, 32, 130, generic=True)])
def test_fused_mc_sweep_equals_generate_then_decode(oracle, monkeypatch, N, K, B, generic):
    """npd_sc_mc_sweep_fused (message -> codeword -> AWGN generated inside the decode kernel, y never
    stored) == npd_mc_generate + npd_sc_decode_mc_sweep: identical msg_hat and counters at every SNR,
    including 25 dB, where the specialised decoder's closed-form subtrees fall back to step-by-step SC
    (regenerated received words).  N <= 64: the fast kernel's GEN mode; N = 4, 128, 256: the generic
    kernel's (K = 200 > 128: two Philox message blocks).  generic (NPD_SC_GENERIC=1, read per call): the generic
    kernel's GEN mode and its msg-only streaming mode at the lengths the fast kernel otherwise takes, three SNR
    points, and both equal to the oracle's decode and count of the generated words."""
    from neural_polar_decoder_amd import PolarCode, reference_polar_code
    from neural_polar_decoder_amd.codes import polar_info_positions
    if K in (22, 200):
        info = polar_info_positions(N, K) if K == 22 else np.sort(np.random.default_rng(3).choice(N, K, replace=False))
        code = PolarCode(int(np.log2(N)), K, F=np.setdiff1d(np.arange(N), info))
    else:
        code = reference_polar_code(N, K)
    assert code.fused_mc_supported() == (N <= 128)  # N = 256: the driver generates y (faster), the ABI still fuses
    snrs = [-1.0, 1.5, 3.0] if generic else [-1.0, 1.5, 3.0, 25.0]
    seed, off, si0 = 13, 12345, 2
    if generic:
        monkeypatch.setenv("NPD_SC_GENERIC", "1")
    y = torch.empty(len(snrs), B, N, device=DEV)
    for i, s in enumerate(snrs):
        code.mc_generate(B, s, seed, si0 + i, off, out=y[i], want_msg=False)
    c1 = torch.zeros(len(snrs), 2, dtype=torch.int64, device=DEV)
    h1 = torch.empty(len(snrs), B, K, device=DEV)
    code.sc_decode_mc_sweep(y, snrs, seed, off, c1, msg_hat=h1)
    c2 = torch.zeros(len(snrs), 2, dtype=torch.int64, device=DEV)
    h2 = torch.empty(len(snrs), B, K, device=DEV)
    code.sc_mc_sweep_fused(B, snrs, seed, off, c2, msg_hat=h2, snr_index0=si0)
    assert torch.equal(h1, h2)
    assert torch.equal(c1, c2), (c1.tolist(), c2.tolist())
    if generic:
        _oracle_sweep_check(oracle, code, code.info_positions, False, y, snrs, seed, off, h2, c2)


def _oracle_sweep_check(oracle, code, info, pac, y, snrs, seed, off, hat, cnt):
    """msg_hat (S, B, K) and counters (S, 2) of a sweep over the received words y (S, B, N) == the oracle's"""
    msg = oracle.gen_msg(y.shape[1], len(info), seed, off)
    for i, s in enumerate(snrs):
        yh = y[i].cpu().numpy()
        oh = oracle.pac_sc_decode(yh, s, info)[1] if pac else oracle.sc_decode(yh, s, info)[1]
        assert np.array_equal(hat[i].cpu().numpy(), oh), s
        assert cnt[i].tolist() == list(oracle.count_errors(msg, oh)), s


@pytest.mark.parametrize("N,K,B,nospec", [(128, 64, 50_001, False), (128, 64, 3001, True), (64, 22, 4097, False),
                                          (32, 16, 999, False), (256, 128, 2000, False), (4, 2, 130, False),
                                          (8, 4, 130, False), (16, 8, 130, False)])
def test_pac_fused_mc_sweep_equals_generate_then_decode(oracle, N, K, B, nospec, monkeypatch):
    """PAC: the generic kernel's GEN mode (msg -> v -> convolution -> Plotkin -> AWGN in registers, PAC SC,
    counts) == npd_mc_generate + npd_sc_decode_mc per SNR point: identical v_hat[:, B] and counters.
    PAC(128,64) 'RM' runs the compile-time frozen-set kernel; nospec forces the run-time frozen set.  The B = 130
    cases (N = 4, 8, 16: kernels no other case reaches) run three SNR points and are also held to the oracle."""
    import argparse
    from neural_polar_decoder_amd import PAC
    if nospec:
        monkeypatch.setenv("NPD_SC_NOSPEC", "1")
    code = PAC(argparse.Namespace(target_K=K), N, K, 91)
    # the C ABI fuses every N; the Monte-Carlo driver takes the fused path up to N = 128 (N = 256 spills)
    assert code.fused_mc_supported() == (N <= 128)
    snrs = [-1.0, 1.0, 2.5] if B == 130 else [-1.0, 1.0, 2.5, 25.0]
    seed, off, si0 = 29, 777, 1
    c1 = torch.zeros(len(snrs), 2, dtype=torch.int64, device=DEV)
    h1 = torch.empty(len(snrs), B, K, device=DEV)
    ys = []
    for i, s in enumerate(snrs):
        _, _, y = code.mc_generate(B, s, seed, si0 + i, off, device=DEV, want_msg=False)
        code.sc_decode_mc(y, s, seed, off, c1[i], msg_hat=h1[i])
        if B == 130:
            ys.append(y)
    c2 = torch.zeros(len(snrs), 2, dtype=torch.int64, device=DEV)
    h2 = torch.empty(len(snrs), B, K, device=DEV)
    code.sc_mc_sweep_fused(B, snrs, seed, off, c2, msg_hat=h2, snr_index0=si0)
    assert torch.equal(h1, h2)
    assert torch.equal(c1, c2), (c1.tolist(), c2.tolist())
    if B == 130:
        _oracle_sweep_check(oracle, code, code.B, True, torch.stack(ys), snrs, seed, off, h2, c2)


def test_fused_mc_argument_checks():
    """Output buffers are validated before the kernel writes through their pointers; more than 16 SNR points
    per call are refused by the C ABI."""
    from neural_polar_decoder_amd import NpdError, reference_polar_code
    code = reference_polar_code(64, 32)
    with pytest.raises(ValueError):
        code.sc_mc_sweep_fused(64, [1.0, 2.0], 1, 0, torch.zeros(1, 2, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        code.sc_mc_sweep_fused(64, [1.0], 1, 0, torch.zeros(1, 2, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        code.sc_mc_sweep_fused(64, [1.0], 1, 0, torch.zeros(1, 2, dtype=torch.int64, device=DEV),
                               msg_hat=torch.empty(63, 32, device=DEV))
    with pytest.raises(NpdError):
        code.sc_mc_sweep_fused(8, [1.0] * 17, 1, 0, torch.zeros(17, 2, dtype=torch.int64, device=DEV))


def test_montecarlo_fused_equals_unfused():
    """SCMonteCarlo with the fused sweep == the generate-then-decode path, counter for counter."""
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.montecarlo import SCMonteCarlo
    code = reference_polar_code(64, 32)
    a = SCMonteCarlo(code, [0.0, 2.0, 4.0], 70_001, 30_000, seed=3).run()
    b = SCMonteCarlo(code, [0.0, 2.0, 4.0], 70_001, 30_000, seed=3, fused=False).run()
    assert a.bit_errors == b.bit_errors and a.block_errors == b.block_errors


def test_count_errors_cols_equals_gather(oracle):
    """npd_count_errors_cols (decisions read at the information columns of the full (B,N) rows) ==
    npd_count_errors on the gathered (B,K) copy == the oracle; zeros count as errors."""
    from neural_polar_decoder_amd.utils import count_errors
    rng = np.random.default_rng(4)
    for B, N, K in [(100_003, 64, 32), (777, 256, 200), (5, 16, 1)]:
        info = np.sort(rng.choice(N, K, replace=False))
        dec = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=(B, N), p=[0.45, 0.1, 0.45])
        msg = (1 - 2 * (rng.random((B, K)) < 0.5)).astype(np.float32)
        c1 = count_errors(t(msg), t(dec), cols=info)
        c2 = count_errors(t(msg), t(np.ascontiguousarray(dec[:, info])))
        assert c1.cpu().tolist() == c2.cpu().tolist() == list(oracle.count_errors(msg, np.ascontiguousarray(dec[:, info])))


def test_ragged_tail_from_exact_size_allocation():
    """The N = 128 streaming kernels (PAC(128,64) 'RM' msg-only, Polar(128,64)) stage a tile by LDS-DMA through a
    buffer descriptor sized to the rows left; rows past B must come back as zeros, never from past the end of y.
    Here y is a bare hipMalloc of exactly B x N floats (no caching-allocator slack behind it), the batch is
    ragged, and the C-ABI is called directly: msg_hat and counts equal those of the same words decoded from a
    torch tensor, and the counts equal the errors against the Philox messages."""
    import ctypes
    from neural_polar_decoder_amd import _lib
    from neural_polar_decoder_amd.polar import llr_scale
    hip = ctypes.CDLL("libamdhip64.so")
    L = _lib.load()
    pac = pac_for(128, 64)
    from neural_polar_decoder_amd import polar_info_positions
    pol = polar_for(128, polar_info_positions(128, 64))
    for code, handle, K in ((pac, pac._code_for(pac.B), 64), (pol, pol.code, 64)):
        for Bn in (3001, 50001, 1):
            msg, _, y = code.mc_generate(Bn, 1.0, 77, 0, 0)
            nbytes = y.numel() * 4
            p = ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
            try:
                torch.cuda.synchronize()
                assert hip.hipMemcpy(p, ctypes.c_void_p(y.data_ptr()), ctypes.c_size_t(nbytes), 3) == 0  # D2D
                cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
                hat = torch.empty(Bn, K, device=DEV)
                _lib.check(L.npd_sc_decode_mc(handle.h, p, llr_scale(1.0), _lib.ptr(hat), 77, 0, Bn, _lib.ptr(cnt),
                                              _lib.stream_of(torch.device(DEV))), "npd_sc_decode_mc")
                torch.cuda.synchronize()
            finally:
                hip.hipFree(p)
            cnt2 = torch.zeros(2, dtype=torch.int64, device=DEV)
            hat2 = torch.empty(Bn, K, device=DEV)
            code.sc_decode_mc(y, 1.0, 77, 0, cnt2, msg_hat=hat2)
            assert torch.equal(hat, hat2) and cnt.tolist() == cnt2.tolist(), (code, Bn)
            e = (hat != msg).sum(1)
            assert cnt.tolist() == [int(e.sum()), int((e > 0).sum())]


@pytest.mark.parametrize("N,K,B", [(64, 32, 4097), (32, 16, 999), (128, 64, 3001), (256, 128, 2000)])
def test_sweep_equals_per_snr_calls(oracle, N, K, B):
    """npd_sc_decode_mc_sweep (one launch over the SNR segments; the bench's streaming step and the N = 256 / non-fused
    Monte-Carlo path) == one npd_sc_decode_mc per SNR point, on ragged batches, and its msg_hat == the oracle's."""
    from neural_polar_decoder_amd import polar_info_positions
    code = polar_for(N, polar_info_positions(N, K))
    snrs = [-1.0, 1.5, 3.0, 25.0]
    seed, off = 17, 4321
    y = torch.empty(len(snrs), B, N, device=DEV)
    for i, s_ in enumerate(snrs):
        code.mc_generate(B, s_, seed, i, off, out=y[i], want_msg=False)
    c1 = torch.zeros(len(snrs), 2, dtype=torch.int64, device=DEV)
    h1 = torch.empty(len(snrs), B, K, device=DEV)
    code.sc_decode_mc_sweep(y, snrs, seed, off, c1, msg_hat=h1)
    for i, s_ in enumerate(snrs):
        c2 = torch.zeros(2, dtype=torch.int64, device=DEV)
        h2 = torch.empty(B, K, device=DEV)
        code.sc_decode_mc(y[i], s_, seed, off, c2, msg_hat=h2)
        assert torch.equal(h1[i], h2), (N, s_)
        assert c1[i].tolist() == c2.tolist(), (N, s_)
    _, oh = oracle.sc_decode(y[1, :512].cpu().numpy(), snrs[1], code.info_positions)
    assert np.array_equal(h1[1, :512].cpu().numpy(), oh)


# every environment switch of the SC kernels, both sides in one process: identical msg_hat and counts
ENV_CASES = [("NPD_SC_GENERIC", "1", "polar", 64, 32), ("NPD_SC_GENERIC", "1", "polar", 32, 16),
             ("NPD_SCF_ILV", "0", "polar", 64, 32), ("NPD_SCF_ILV", "1", "polar", 64, 32),
             ("NPD_SCF_WPB", "1", "polar", 64, 32), ("NPD_SCF_WPB", "4", "polar", 16, 8),
             ("NPD_SC_NOSPEC", "1", "polar", 64, 32), ("NPD_SC_ROOT", "0", "pac", 128, 64),
             ("NPD_SC_NOSPEC", "1", "pac", 128, 64)]


@pytest.mark.parametrize("var,val,kind,N,K", ENV_CASES)
def test_env_switches_decode_identically(monkeypatch, var, val, kind, N, K):
    from neural_polar_decoder_amd import polar_info_positions
    code = pac_for(N, K) if kind == "pac" else polar_for(N, polar_info_positions(N, K))
    B = 5003
    msg, _, y = code.mc_generate(B, 1.0, 91, 0, 0)
    snrs = [0.5, 2.0]

    def run():
        cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
        hat = torch.empty(B, K, device=DEV)
        code.sc_decode_mc(y, 1.0, 91, 0, cnt, msg_hat=hat)
        c2 = torch.zeros(len(snrs), 2, dtype=torch.int64, device=DEV)
        h2 = torch.empty(len(snrs), B, K, device=DEV)
        code.sc_mc_sweep_fused(B, snrs, 91, 0, c2, msg_hat=h2)
        return hat, cnt.tolist(), h2, c2.tolist()

    base = run()
    monkeypatch.setenv(var, val)
    alt = run()
    monkeypatch.delenv(var)
    assert torch.equal(base[0], alt[0]) and base[1] == alt[1]
    assert torch.equal(base[2], alt[2]) and base[3] == alt[3]
    e = (base[0] != msg).sum(1)
    assert base[1] == [int(e.sum()), int((e > 0).sum())]
