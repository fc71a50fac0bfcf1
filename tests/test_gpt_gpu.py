"""GPU: the fused GPT transformer decode (npd_gpt_decode) against the float64 restatement and the reference's bits.

tol = max(2e-5, 4 e_ref) per fixture (tests/test_gpt.py explains it); every float64 result is computed once per session
in tests/gpt_helper.py and shared.
"""
import argparse
import os

import numpy as np
import pytest
import torch

import gpt_helper as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_NETS = {}


def net_of(name):
    if name not in _NETS:
        _NETS[name] = G.build_net(name, DEV)
    return _NETS[name]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.mark.parametrize("name", G.FIXTURES)
def test_forced_path_logits_against_float64(name):
    """Every fixture, word and information step; the bits returned are the signs of the logits."""
    d, _ = G.fixture(name)
    info = d["info"]
    bits, lg = net_of(name).decode_logits(t(d["y_forced"]), info, forced=t(d["forced"]))
    lg, bits = lg.cpu().numpy().astype(np.float64), bits.cpu().numpy()
    err = np.abs(lg - G.forced64(name))[:, info]
    print(f"{name}: max |kernel - float64| {err.max():.3g} (tol {G.tol_of(d):.3g}, reference's own {float(d['e_ref']):.3g})")
    assert err.max() <= G.tol_of(d)
    frozen = np.setdiff1d(np.arange(int(d["N"])), info)
    assert np.all(lg[:, frozen] == 0) and np.all(bits[:, frozen] == 1)
    assert np.array_equal(bits[:, info], np.sign(lg[:, info]))


@pytest.mark.parametrize("name", G.FIXTURES)
def test_free_decode_against_the_reference(name):
    """The reference's bits on the robust words (min |logit64| >= 10 tol); logits within tol wherever the decided paths
    agree with the float64 decode's (all earlier information bits equal)."""
    d, _ = G.fixture(name)
    info, tol = d["info"], G.tol_of(d)
    y = t(d["y"])
    dec, mask = net_of(name).decode(y, info, torch.ones_like(y).long(), DEV)
    bits, lg = net_of(name).decode_logits(y, info)
    assert torch.equal(dec, bits) and mask.shape == y.shape and bool(mask.all())
    bits, lg = bits.cpu().numpy(), lg.cpu().numpy().astype(np.float64)
    b64, l64 = G.free64(name)
    robust = np.abs(l64[:, info]).min(1) >= 10 * tol
    assert robust.sum() >= 0.9 * len(robust)
    assert np.array_equal(bits[robust], d["ref_bits"][robust].astype(np.float32))
    same = bits[:, info] == b64[:, info]
    agree = np.concatenate([np.ones((len(same), 1), bool), np.cumprod(same, 1)[:, :-1].astype(bool)], 1)
    err = np.abs(lg - l64)[:, info][agree]
    print(f"{name}: {int(robust.sum())} robust words of {len(robust)}, {int(agree.sum())} steps on agreeing paths, "
          f"max |kernel - float64| {err.max():.3g} (tol {tol:.3g})")
    assert err.max() <= tol


@pytest.mark.parametrize("name", [G.FIXTURES[0], G.FIXTURES[1], G.FIXTURES[2]])
def test_rows_do_not_depend_on_the_batch(name):
    """B = 1, 5, 33, 70 (partial workgroups, one and many): bit-identical to the same rows of the full batch."""
    d, _ = G.fixture(name)
    info = d["info"]
    y = t(np.concatenate([d["y"], d["y_forced"]]))
    net = net_of(name)
    fb, fl = net.decode_logits(y, info)
    for B in (1, 5, 33, 70):
        b, l = net.decode_logits(y[:B].clone(), info)
        assert torch.equal(b, fb[:B]) and torch.equal(l, fl[:B]), B
    b, l = net.decode_logits(y[:0], info)
    assert b.shape == (0, int(d["N"])) and l.shape == (0, int(d["N"]))


@pytest.mark.parametrize("name", [G.FIXTURES[0], G.FIXTURES[1], G.FIXTURES[4]])
def test_custom_information_set_with_both_ends(name):
    """Positions 0 (prefix length 1) and N - 1 (the last step) among the information positions."""
    d, sd = G.fixture(name)
    N = int(d["N"])
    info = np.array([0, 1, 2, N // 2 - 1, N // 2, N - 2, N - 1])
    is_info = np.zeros(N, np.uint8)
    is_info[info] = 1
    n = 16
    y, forced = d["y_forced"][:n], d["forced"][:n]
    _, l64 = G.decode64(sd, y, is_info, forced=forced)
    bits, lg = net_of(name).decode_logits(t(y), torch.as_tensor(info), forced=t(forced))
    lg = lg.cpu().numpy().astype(np.float64)
    err = np.abs(lg - l64)
    print(f"{name}: info {info.tolist()}, max |kernel - float64| {err.max():.3g} (tol {G.tol_of(d):.3g})")
    assert err.max() <= G.tol_of(d)
    assert np.all(lg[:, is_info == 0] == 0) and np.all(lg[:, info] != 0)


def test_host_tensors_come_home():
    name = G.FIXTURES[0]
    d, _ = G.fixture(name)
    y = torch.from_numpy(d["y"][:8])
    bits, lg = net_of(name).decode_logits(y, d["info"])
    assert not bits.is_cuda and not lg.is_cuda
    gb, gl = net_of(name).decode_logits(y.to(DEV), d["info"])
    assert torch.equal(gb.cpu(), bits) and torch.equal(gl.cpu(), lg)


def test_testXformer_replay():
    """run_models.py:318-345 with the default --model gpt: the loop of tests/test_eval_loops_gpu.py, the class swapped in.
    The transformer's block-error rate equals the float64 decode's of the recorded words up to the words that are not
    robust (min |logit64| < 10 tol)."""
    from neural_polar_decoder_amd import reference_polar_code
    from test_eval_loops_gpu import replay_testXformer
    name = G.FIXTURES[1]
    d, sd = G.fixture(name)
    polar = reference_polar_code(32, 16)
    polar.manual_seed(11)
    B = 64
    g = torch.Generator().manual_seed(3)
    batches = [1 - 2 * torch.randint(0, 2, (B, 16), generator=g).float()]
    snrs = [1.0, 3.0]
    rec = []
    bers_X, blers_X = replay_testXformer(net_of(name), polar, snrs, batches, DEV, rec)[:2]
    info = np.asarray(polar.info_positions)
    is_info = np.zeros(32, np.uint8)
    is_info[info] = 1
    for (msg, y, snr), ber, bler in zip(rec, bers_X, blers_X):
        b64, l64 = G.decode64(sd, y, is_info)
        loose = int((np.abs(l64[:, info]).min(1) < 10 * G.tol_of(d)).sum())
        wrong = (b64[:, info] != msg).any(1).mean()
        assert abs(bler - wrong) <= loose / B + 1e-9
        assert isinstance(ber, float) and 0.0 <= ber <= 1.0


def test_monte_carlo_counts_equal_decode_and_count():
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.montecarlo import GPTMonteCarlo, seeded_gpt
    from neural_polar_decoder_amd.utils import count_errors
    code = reference_polar_code(32, 16)
    net = seeded_gpt(32, 2, seed=4, device=DEV)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 2:
                p.mul_(G.INIT_SCALE)
    snrs = [0.0, 2.0]
    mc = GPTMonteCarlo(code, net, snrs, 300, 128, seed=7, device=DEV)
    res = mc.run()
    exp = torch.zeros(len(snrs), 2, dtype=torch.int64, device=DEV)
    for si, snr in enumerate(snrs):
        for off in range(0, 300, 128):
            n = min(128, 300 - off)
            msg, y = mc.generate(si, snr, off, n)
            bits, _ = net.decode(y, code.info_positions, torch.ones_like(y).long(), DEV)
            count_errors(msg, bits, exp[si], cols=np.asarray(code.info_positions))
    got = res.as_dict()
    assert got["bit_errors"] == exp[:, 0].cpu().tolist() and got["block_errors"] == exp[:, 1].cpu().tolist()
    assert sum(got["block_errors"]) > 0


def test_checkpoint_round_trip(tmp_path):
    from neural_polar_decoder_amd.datasets import xformer_from_checkpoint
    name = G.FIXTURES[1]
    d, sd = G.fixture(name)
    args = G.gpt_config(32, 2)
    args.K, args.code = 16, "polar"
    path = os.path.join(tmp_path, "gpt.pt")
    torch.save({"xformer": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "args": args, "step": 1}, path)
    net = xformer_from_checkpoint(path, device=DEV)
    assert not net.training and net.fused_supported()
    y = t(d["y"][:32])
    b, l = net.decode_logits(y, d["info"])
    rb, rl = net_of(name).decode_logits(y, d["info"])
    assert torch.equal(b, rb) and torch.equal(l, rl)
