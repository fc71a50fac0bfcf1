"""Every RNN decode kernel against float64 along forced paths, on the MI355X (forced_helper.CASES: one case per
instantiated decode kernel -- gru_decode_kernel, gru_decode_bf_kernel, gru16p_kernel, gru_wide_kernel,
lstm_decode_kernel, lstm_wide_kernel -- and the y_h0 route of five of them; forced_helper.LONG_CASES: every family at
N = 256, at lengths that are no power of two, and at N = 248 where F = 512 x 2 layers fills the LDS).

Each case runs three decodes through RNN_decoder.decode: A fully forced (gt random +-1, loss_inds []), B genie
(loss_inds the information set, gt's frozen entries from {-1, +1, 0, -0.3, 2.5}; two cases also with loss_inds = every
other position) and C plain (gt None).  Each is verified along the path it reports: float64
(oracle.gru_decode_f64) forced along step_path(decoded), then forced_helper.check_forced over ALL words and steps, none
excluded: |kernel logit - float64 logit| < bar, decoded at loss positions exactly sign(kernel logit), decoded elsewhere
bitwise gt (1.0 without gt), logits finite.  The bars are the project's own per family (fp32 GRU narrow and wide, fp32
narrow LSTM, fp16x3: 2e-5; lstm_wide_kernel: 5e-5; bf16x3: 2e-3).  Precision bf16 has no logit bar in this project: for
its cases the three exact properties are asserted and the error is only printed.  Each test prints max err, E_ref (the
reference's own fp32 arithmetic against float64 on the forced decode) and their ratio; the table is in DESIGN.md 2c.
tests/test_forced_path.py holds the conditions that make these bars fair and these inputs sharp.
"""
import ctypes

import numpy as np
import pytest
import torch

import forced_helper as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}
# one case per family at its smallest length and one at N = 256
FAMILY_CASES = list(H.FAMILY_CASE.values()) + list(H.LONG_FAMILY_CASE.values())


def setup(case):
    """(CPU net, GPU net, state dict, decoder) of a case, built once."""
    from neural_polar_decoder_amd.rnn import RNN_decoder
    if case.id not in _cache:
        net = H.build_net(case)
        gnet = H.build_net(case, DEV)
        dec = RNN_decoder("y_h0" if case.yh0 else "y_input", case.N, H.info_set(case.N), onehot=case.onehot,
                          reverse_order=case.rev, precision=case.precision)
        _cache[case.id] = (net, gnet, H.state_dict_np(net), dec)
    return _cache[case.id]


def run(case, gnet, dec, y, gt, loss):
    out, lg = dec.decode(gnet, False, torch.from_numpy(y).to(DEV), gt=None if gt is None else torch.from_numpy(gt).to(DEV),
                         loss_inds=loss, return_logits=True)
    return out.cpu().numpy(), lg.cpu().numpy()


def verify(case, sd, y, gt, loss, dec_k, lg_k):
    l64 = H.f64_forced(case, sd, y, H.step_path(dec_k, case.rev))
    return H.check_forced(lg_k, dec_k, gt, loss, l64, case.bar, case.rev)


@pytest.mark.parametrize("case", H.CASES + H.LONG_CASES, ids=lambda c: c.id)
def test_decode_along_its_own_path(case):
    net, gnet, sd, dec = setup(case)
    errs = {}
    modes = [("A", "forced", False), ("B", "genie", False), ("C", "plain", False)]
    if case.id in H.ALTERNATE_LOSS:
        modes.append(("B'", "genie", True))
    for tag, mode, alt in modes:
        y, gt, loss = H.make_inputs(case, mode, alternate=alt)
        dec_k, lg_k = run(case, gnet, dec, y, gt, loss)
        errs[tag] = verify(case, sd, y, gt, loss, dec_k, lg_k)
        if tag == "A":
            path = H.step_path(dec_k, case.rev)
            e_ref = np.abs(H.ref32_forced(net, case, y, path) - H.f64_forced(case, sd, y, path)).max()
    worst = max(errs.values())
    print(f"FORCED {case.id} | {case.family} | g {case.g} | ys {case.ys:.4f} | bar {case.bar} | max err {worst:.2e} | "
          f"E_ref {e_ref:.2e} | ratio {worst / e_ref:.2f} | " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))


@pytest.mark.parametrize("case", FAMILY_CASES, ids=lambda c: c.id)
def test_negative_control_breaks_the_bar(case):
    """The comparison has teeth end to end: the kernel decodes with weight_hh_l0's last column zeroed (a dropped k element
    of the recurrent product, as weights: the same code on other numbers) and is compared with the UNMUTATED float64
    logits along the same forced path; at least half the words must break the bar."""
    net, gnet, sd, dec = setup(case)
    mnet = H.load_np(H.build_net(case), H.MUTATIONS[H.NEGATIVE_CONTROL](sd, case)).to(DEV).eval()
    y, gt, loss = H.make_inputs(case, "forced")
    dec_k, lg_k = run(case, mnet, dec, y, gt, loss)
    assert np.array_equal(dec_k.view(np.uint32), gt.view(np.uint32))
    err = np.abs(lg_k - H.f64_forced(case, sd, y, H.step_path(dec_k, case.rev))).max(1)
    print(f"CONTROL {case.id}: words over the bar {(err >= case.bar).mean():.2f}, median {np.median(err) / case.bar:.0f} bars")
    assert (err >= case.bar).mean() >= 0.5
    with pytest.raises(AssertionError):
        verify(case, sd, y, gt, loss, dec_k, lg_k)


@pytest.mark.parametrize("case", FAMILY_CASES, ids=lambda c: c.id)
def test_single_word_batch(case):
    """B = 1: every lane of the tile but one is clamped to row B - 1."""
    net, gnet, sd, dec = setup(case)
    for mode in ("forced", "genie", "plain"):
        y, gt, loss = H.make_inputs(case, mode, B=1)
        dec_k, lg_k = run(case, gnet, dec, y, gt, loss)
        assert dec_k.shape == (1, case.N)
        verify(case, sd, y, gt, loss, dec_k, lg_k)


@pytest.mark.parametrize("case", FAMILY_CASES, ids=lambda c: c.id)
def test_rows_past_the_batch_are_untouched(case):
    """npd_gru_decode_ex called directly with decoded / logits the first B = 70 rows of buffers 32 rows longer that hold a
    sentinel bit pattern: the 32 trailing rows of both stay bitwise unchanged, the first B rows are the decode."""
    from neural_polar_decoder_amd import _lib
    net, gnet, sd, dec = setup(case)
    B, N, PAD = 70, case.N, 32
    y, gt, loss = H.make_inputs(case, "genie", B=B)
    want_dec, want_lg = run(case, gnet, dec, y, gt, loss)
    sentinel = 0x7FC5A5A5  # a NaN payload: no arithmetic produces it
    bufs = [torch.full((B + PAD, N), sentinel, dtype=torch.int32, device=DEV) for _ in range(2)]
    yd, gd = torch.from_numpy(y).to(DEV), torch.from_numpy(gt).to(DEV)
    is_info = np.zeros(N, np.uint8)
    is_info[loss] = 1
    h = dec._handle(gnet, torch.device(DEV))
    rc = _lib.load().npd_gru_decode_ex(h.h, _lib.ptr(yd), None, is_info.ctypes.data_as(ctypes.c_void_p),
                                       1 if case.rev else 0, _lib.ptr(gd), _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), B,
                                       _lib.stream_of(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    got = [b.cpu().numpy() for b in bufs]
    for g, want in zip(got, (want_dec, want_lg)):
        assert np.all(g[B:] == sentinel), "a row past B was written"
        assert np.array_equal(g[:B].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", H.FIXTURES)
def test_reference_fixture_logits_along_recorded_decisions(name):
    """Mode A along the reference's recorded decisions (gt = the recorded decoded, raw frozen values included,
    loss_inds []): the kernel's logits are within the bar of the logits the reference recorded, on every word."""
    from neural_polar_decoder_amd.rnn import RNN_decoder
    case, d, sd = H.load_fixture(name)
    gnet = H.load_np(H.build_net(case), sd).to(DEV).eval()
    dec = RNN_decoder("y_input", case.N, d["info"], onehot=case.onehot, reverse_order=case.rev)
    gt = np.ascontiguousarray(d["decoded"], np.float32)
    dec_k, lg_k = run(case, gnet, dec, d["y"], gt, np.zeros(0, np.int64))
    assert np.array_equal(dec_k.view(np.uint32), gt.view(np.uint32))
    err = np.abs(lg_k.astype(np.float64) - d["logits"])
    print(f"FIXTURE {name}: max |kernel - reference| {err.max():.2e} (bar {case.bar})")
    assert np.all(np.isfinite(lg_k)) and err.max() < case.bar
    # and the genie decode of the recorded inputs, verified along its own path like every other
    dec_g, lg_g = run(case, gnet, dec, d["y"], d["gt"], d["info"])
    verify(case, sd, d["y"], d["gt"], d["info"], dec_g, lg_g)
