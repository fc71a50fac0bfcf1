"""The conditions on the inputs of the forced-path GPU tests (tests/test_forced_path_gpu.py), on the CPU.

They keep the GPU test from being toothless or unfair, for every row of forced_helper.CASES and LONG_CASES:
  * E_ref <= bar / 4: the reference's own arithmetic (torch fp32 on the CPU, one net(...) call per step) is within a
    quarter of the bar of float64, on the fully forced path and on its own genie path -- so the bar is one the reference
    passes with room to spare;
  * every applicable entry of MUTATIONS (typical kernel faults restated as weight edits) moves the float64 logits by
    >= 10 bars at some step of at least half the words -- so a kernel with that fault cannot pass;
  * the C oracle's genie branch (oracle.gru_decode(..., gt=, rev=)), the yardstick of the list-decoding tests, is held
    to float64 along its own path;
  * step_path / reverse bookkeeping: forcing float64 along its own autoregressive output reproduces its logits exactly;
  * the fixtures recorded from the reference (tests/golden/gen_forced.py) are reproduced by float64 within bar / 4 and
    obey the raw-gt / loss_inds / reverse semantics the helper restates.
Plain bf16 has no logit bar in this project: its cases share net, words and scale rule with the bf16x3 case of the same
shape, and only the exact properties are asserted for them on the GPU.
"""
import numpy as np
import pytest

import forced_helper as H

BARRED = [c for c in H.CASES + H.LONG_CASES if c.bar is not None]
_cache = {}


def setup(case):
    """(net, state dict, forced inputs, float64 logits along the forced path), computed once per case."""
    if case.id not in _cache:
        net = H.build_net(case)
        sd = H.state_dict_np(net)
        y, gt, _ = H.make_inputs(case, "forced")
        path = H.step_path(gt, case.rev)
        l64 = H.f64_forced(case, sd, y, path)
        l64.setflags(write=False)
        _cache[case.id] = (net, sd, y, path, l64)
    return _cache[case.id]


def test_case_table_reaches_every_decode_instantiation():
    """47 instantiated decode kernels: gru_decode_kernel (F, L) x head tiling {0, 1, 2, 4}, gru_decode_bf_kernel (F, L) x
    split, gru16p_kernel x split, gru_wide_kernel and lstm_decode_kernel / lstm_wide_kernel (F, L)."""
    inst = set()
    for c in H.CASES:
        if c.family == "gru_decode_kernel":
            w = c.head[1] if isinstance(c.head, tuple) else 0
            inst.add((c.family, c.F, c.layers, 0 if w == 0 else 1 if w <= 32 else 2 if w <= 64 else 4))
        elif c.family in ("gru_decode_bf_kernel", "gru16p_kernel"):
            assert c.family == ("gru16p_kernel" if c.F == 64 and c.layers == 2 and c.N % 32 == 0 else "gru_decode_bf_kernel")
            inst.add((c.family, c.F, c.layers, c.precision))
        else:
            inst.add((c.family, c.F, c.layers))
        if c.cell == "LSTM":  # npd_gru_decode_ex's route
            assert c.family == ("lstm_decode_kernel" if c.F * c.layers <= 64 else "lstm_wide_kernel")
        elif c.precision == "fp32":
            assert c.family == ("gru_wide_kernel" if c.F > 64 else "gru_decode_kernel")
    assert len(inst) == 47
    for f in H.FAMILIES:  # both values of onehot and of reverse_order in every family
        assert {c.onehot for c in H.CASES if c.family == f} == {False, True}, f
        assert {c.rev for c in H.CASES if c.family == f} == {False, True}, f
    assert len({c.id for c in H.CASES}) == len(H.CASES)
    assert set(H.ALTERNATE_LOSS) <= set(H.CASE_BY_ID)


def test_long_case_table():
    """LONG_CASES: N = 256 in every family, lengths that are no power of two, N = 248 at F = 512 x 2 (the LDS exactly
    full) on both wide kernels, odd K-block counts and the y_h0 route on gru16p_kernel; every case has a bar; both
    values of onehot and of reverse_order in every family; the route of every case is the family it names; g and the
    y scale are recorded per case."""
    assert not set(c.id for c in H.CASES) & set(c.id for c in H.LONG_CASES)
    assert len({c.id for c in H.LONG_CASES}) == len(H.LONG_CASES) and all(c.ys == 1.0 for c in H.CASES)
    have = {(c.family, c.F, c.layers, c.precision, c.N, c.yh0) for c in H.LONG_CASES}
    need = [("gru_decode_kernel", 64, 2, "fp32", 256), ("gru_decode_kernel", 32, 1, "fp32", 256),
            ("gru_decode_kernel", 64, 1, "fp32", 24), ("gru_decode_bf_kernel", 32, 2, "fp16x3", 256),
            ("gru_decode_bf_kernel", 32, 2, "bf16x3", 256), ("gru_decode_bf_kernel", 64, 1, "fp16x3", 256),
            ("gru_decode_bf_kernel", 64, 1, "bf16x3", 256), ("gru_decode_bf_kernel", 32, 1, "fp16x3", 48),
            ("gru16p_kernel", 64, 2, "fp16x3", 256), ("gru16p_kernel", 64, 2, "bf16x3", 256),
            ("gru16p_kernel", 64, 2, "fp16x3", 96), ("gru16p_kernel", 64, 2, "fp16x3", 160),
            ("gru_wide_kernel", 128, 2, "fp32", 256), ("gru_wide_kernel", 512, 1, "fp32", 256),
            ("gru_wide_kernel", 256, 1, "fp32", 40), ("gru_wide_kernel", 512, 2, "fp32", 248),
            ("lstm_decode_kernel", 32, 2, "fp32", 256), ("lstm_decode_kernel", 64, 1, "fp32", 256),
            ("lstm_wide_kernel", 256, 2, "fp32", 256), ("lstm_wide_kernel", 512, 2, "fp32", 248)]
    for row in need:
        assert row + (False,) in have, row
    assert ("gru16p_kernel", 64, 2, "fp16x3", 256, True) in have
    for c in H.LONG_CASES:
        assert c.bar == H.bar_of(c.family, c.precision) and c.bar is not None and c.head is None
        assert c.B == (24 if c.F == 512 else 70) and 8 <= c.N <= 256 and c.N % 8 == 0
        assert c.g > 0 and (c.ys == 1.0 or (not c.yh0 and np.isclose(c.ys, np.sqrt(16 / c.N))))
        if c.cell == "LSTM":
            assert c.precision == "fp32" and c.family == ("lstm_decode_kernel" if c.F * c.layers <= 64 else "lstm_wide_kernel")
        elif c.precision == "fp32":
            assert c.family == ("gru_wide_kernel" if c.F > 64 else "gru_decode_kernel")
        else:
            assert c.N % 16 == 0
            assert c.family == ("gru16p_kernel" if c.F == 64 and c.layers == 2 and c.N % 32 == 0 else "gru_decode_bf_kernel")
        if c.F == 512 and c.layers == 2:  # gru::wide_lds_bytes: all 160 KiB
            assert (c.layers * c.F + c.N + 8) * 128 == 160 * 1024
    for f in H.FAMILIES:
        assert {c.onehot for c in H.LONG_CASES if c.family == f} == {False, True}, f
        assert {c.rev for c in H.LONG_CASES if c.family == f} == {False, True}, f
        assert H.LONG_FAMILY_CASE[f].family == f and H.LONG_FAMILY_CASE[f].N == 256
    for N in (24, 40, 48, 96, 160, 248):  # no code of the reference: a seeded half of the positions
        info = H.info_set(N)
        assert info.size == N // 2 and np.array_equal(info, np.unique(info)) and 0 <= info[0] and info[-1] < N
        assert np.array_equal(info, H.info_set(N))


@pytest.mark.parametrize("case", BARRED, ids=lambda c: c.id)
def test_reference_arithmetic_is_within_a_quarter_of_the_bar(case):
    net, sd, y, path, l64 = setup(case)
    e_forced = np.abs(H.ref32_forced(net, case, y, path) - l64).max()
    yg, gt, loss = H.make_inputs(case, "genie")
    dec, lg = H.ref32_decode(net, case, yg, gt, loss)
    e_genie = H.check_forced(lg, dec, gt, loss, H.f64_forced(case, sd, yg, H.step_path(dec, case.rev)), case.bar / 4,
                             case.rev)
    print(f"{case.id}: E_ref forced {e_forced:.2e} genie {e_genie:.2e} bar {case.bar:.0e} max |logit| {np.abs(l64).max():.2f}")
    assert e_forced <= case.bar / 4, (e_forced, case.bar)
    assert np.abs(l64).max() >= 1.0  # the nets are not tame: logits of order 1 and above


@pytest.mark.parametrize("case", BARRED, ids=lambda c: c.id)
def test_every_mutation_moves_float64_by_ten_bars_on_half_the_words(case):
    net, sd, y, path, l64 = setup(case)
    applied = 0
    for name, fn in H.MUTATIONS.items():
        msd = fn(sd, case)
        if msd is None:
            continue
        applied += 1
        reach = H.mutation_reach(l64, H.f64_forced(case, msd, y, path))
        share = (reach >= 10 * case.bar).mean()
        if (case.id, name) in H.MUTATION_EXCEPTIONS:
            assert share < 0.5, f"{case.id} / {name} reaches 10 bars: take it out of MUTATION_EXCEPTIONS"
        else:
            assert share >= 0.5, f"{case.id} / {name}: only {share:.2f} of the words move by 10 bars " \
                                 f"(median {np.median(reach):.2e}, bar {case.bar:.0e})"
    # which edits apply is a matter of the shape alone
    expect = 2 + (2 if case.layers == 2 else 0) + (0 if case.yh0 else 1) + int(case.onehot) + int(case.cell == "GRU")
    assert applied == expect, (applied, expect)


def test_mutation_exceptions_name_real_pairs():
    for (cid, name), why in H.MUTATION_EXCEPTIONS.items():
        assert cid in H.CASE_BY_ID and H.CASE_BY_ID[cid].bar is not None and name in H.MUTATIONS and why


PLAIN = {(c.F, c.layers, c.N, c.onehot, c.rev, c.seed): c for c in H.CASES
         if c.cell == "GRU" and c.head is None and not c.yh0 and c.F <= 128}


@pytest.mark.parametrize("case", list(PLAIN.values()), ids=lambda c: c.id)
def test_c_oracle_genie_branch_against_float64(case, oracle):
    """oracle.gru_decode with gt (fully forced, genie, genie over every other position) and without, each verified along
    the path it reports, at the fp32 bar 2e-5."""
    net, sd, _, _, _ = setup(case)
    for mode, alt in (("forced", False), ("genie", False), ("genie", True), ("plain", False)):
        y, gt, loss = H.make_inputs(case, mode, alternate=alt)
        dec, lg = oracle.gru_decode(y, sd, case.N, case.F, case.layers, loss, onehot=case.onehot, rev=case.rev, gt=gt,
                                    want_logits=True)
        l64 = H.f64_forced(case, sd, y, H.step_path(dec, case.rev))
        H.check_forced(lg, dec, gt, loss, l64, 2e-5, case.rev)


@pytest.mark.parametrize("cid", ["gru_decode-f32x1", "gru_decode-f32x2", "gru_decode-f64x1-ln", "lstm_decode-f32x2",
                                 "gru_decode-f64x2-d3h48", "gru_wide-f128x1-yh0"])
def test_forcing_float64_along_its_own_output_reproduces_it(cid):
    from oracle import oracle as O
    case = H.CASE_BY_ID[cid]
    net, sd, y, _, _ = setup(case)
    info = H.info_set(case.N)
    h0x = O.ymlp_f64(y, sd, H.YH0_ACT, H.YH0_DEPTH) if case.yh0 else None
    dec, lg = O.gru_decode_f64(y, sd, case.N, case.F, case.layers, info, onehot=case.onehot, h0x=h0x, rev=case.rev,
                               cell=case.cell, ln_eps=H.LN_EPS if case.head == "ln" else None)
    assert np.array_equal(H.f64_forced(case, sd, y, H.step_path(dec, case.rev)), lg)
    assert H.check_forced(lg, dec, None, info, lg, 1e-300, case.rev) == 0.0
    if case.rev:  # the bookkeeping matters: read in position order instead, the path is another one
        assert not np.array_equal(H.f64_forced(case, sd, y, np.sign(dec)), lg)


def test_step_path():
    d = np.array([[2.5, -0.3, 0.0, -1.0]])
    assert np.array_equal(H.step_path(d, False), [[1.0, -1.0, 0.0, -1.0]])
    assert np.array_equal(H.step_path(d, True), [[-1.0, 0.0, -1.0, 1.0]])


@pytest.mark.parametrize("name", H.FIXTURES)
def test_reference_fixture_is_reproduced(name):
    """The reference's recorded genie decode: float64 forced along the recorded decisions is within bar / 4 of the
    recorded logits; decoded holds sign(recorded logit) at the information positions and gt's raw value elsewhere, in
    position order under reverse_order; frozen values of every kind occur, so each feedback rule is exercised."""
    case, d, sd = H.load_fixture(name)
    gt, dec, info = d["gt"], d["decoded"], d["info"]
    l64 = H.f64_forced(case, sd, d["y"], H.step_path(dec, case.rev))
    e = H.check_forced(d["logits"], dec, gt, info, l64, case.bar / 4, case.rev)
    print(f"{name}: |reference - float64| max {e:.2e}")
    frozen = np.setdiff1d(np.arange(case.N), info)
    assert set(np.unique(gt[:, frozen]).tolist()) == set(np.asarray(H.FROZEN_VALUES, np.float32).tolist())
    # this package's restatement of the loop gives the reference's decisions and logits to rounding
    net = H.load_np(H.build_net(case), sd)
    dec32, lg32 = H.ref32_decode(net, case, d["y"], gt, info)
    assert np.array_equal(dec32, dec) and np.abs(lg32 - d["logits"]).max() <= case.bar / 4
    # taking gt the wrong way round under reverse_order, or feeding 0 as +1, is another path: float64 leaves the bar
    wrong = np.where(H.step_path(dec, case.rev) == 0.0, 1.0, H.step_path(dec, case.rev))
    assert np.abs(H.f64_forced(case, sd, d["y"], wrong) - d["logits"]).max() > 10 * case.bar
    if case.rev:
        assert np.abs(H.f64_forced(case, sd, d["y"], np.sign(dec)) - d["logits"]).max() > 10 * case.bar


def test_check_forced_rejects_what_it_should():
    """check_forced has teeth of its own: one logit off by a bar, one decision against its logit's sign, one frozen value
    changed in the last bit, one non-finite logit."""
    rng = np.random.default_rng(3)
    l64 = rng.standard_normal((5, 8))
    lg = l64.astype(np.float32)
    loss = [1, 3, 4, 6]
    gt = np.asarray(H.FROZEN_VALUES, np.float32)[rng.integers(0, 5, (5, 8))]
    for rev in (False, True):
        dec = gt.copy()
        lp = lg[:, ::-1] if rev else lg
        dec[:, loss] = np.sign(lp[:, loss])
        H.check_forced(lg, dec, gt, loss, l64, 2e-5, rev)
        bad = lg.copy()
        bad[4, 7] += 3e-5
        with pytest.raises(AssertionError):
            H.check_forced(bad, dec, gt, loss, l64, 2e-5, rev)
        bad = dec.copy()
        bad[2, 3] = -bad[2, 3]
        with pytest.raises(AssertionError):
            H.check_forced(lg, bad, gt, loss, l64, 2e-5, rev)
        bad = dec.copy()
        bad[0, 0] = np.nextafter(bad[0, 0], np.float32(9.0))
        with pytest.raises(AssertionError):
            H.check_forced(lg, bad, gt, loss, l64, 2e-5, rev)
        bad = lg.copy()
        bad[1, 1] = np.inf
        with pytest.raises(AssertionError):
            H.check_forced(bad, dec, gt, loss, l64, None, rev)
