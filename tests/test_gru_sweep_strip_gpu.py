"""The count sweep's stripped step loop (gru16p_kernel's count-only instantiation, the per-step table in LDS, the
decision skipped at frozen positions, the batched prologue loads): the counters are what they were.

Bars, all exact (integer counters, +-1 decisions):
  1. the counters of tests/golden/gru_sweep_parent_counts.npz, recorded by tests/golden/gen_gru_sweep_parent.py on
     the commit before the step loop changed -- arithmetic drift shows even where fused and unfused drift together;
  2. the unfused sequence, per segment RNN_decoder.decode + count_errors on the same columns;
  3. the general instantiation (decode_count_sweep with `decoded`), whose decisions are RNN_decoder.decode's.
Shapes: more than one tile per wave, ragged last tiles, a counter flush at every segment change, reverse order (whose
trailing steps are all frozen), N = 32 / 64 / 128 (1 / 2 / 4 K blocks of the y projection, K = 16 / 32 / 64 message
slots), the three split instantiations.

Past 64 message columns (test_message_registers_and_slot_255): the message codes of a codeword sit in four registers
of 64 columns each, and every trained case above has K <= 64, the first register alone.  Seeded nets at (N, K) = (96, 96),
(160, 160), (256, 200) and (256, 256) reach the second, third and fourth register and message column 255; the count-only
launch, the general instantiation and the unfused sequence must give the same counters, also after one message column
at a register boundary is negated."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden, trained_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (net, precision, reverse, SNRs (one segment each), B)
CASES = {
    "c32_nat": ("trained_crisp_32_16", "fp16x3", False, [0.0, 1.0, 2.0, 3.0, 4.0], 16 * 700 + 5),
    "c32_rev": ("trained_crisp_32_16", "fp16x3", True, [0.0, 1.0, 2.0, 3.0, 4.0], 16 * 700 + 5),
    "c64_nat": ("trained_crisp_64_32", "fp16x3", False, [0.0, 2.0, 4.0], 16 * 130 + 7),
    "c64_rev": ("trained_crisp_64_32", "fp16x3", True, [0.0, 2.0, 4.0], 16 * 130 + 7),
    "pac128": ("pac_128_64", "fp16x3", False, [0.0, 4.0], 2048 + 9),
    "c32_bf16x3": ("trained_crisp_32_16", "bf16x3", False, [0.0, 1.0, 2.0, 3.0, 4.0], 16 * 700 + 5),
    "c32_bf16": ("trained_crisp_32_16", "bf16", False, [0.0, 1.0, 2.0, 3.0, 4.0], 16 * 700 + 5),
}
PINNED = ["c32_nat", "c32_rev", "c64_nat", "c64_rev", "pac128"]


def words(code, snrs, B, seed=11):
    ys, msg = [], None
    for si, s in enumerate(snrs):
        m, _, y = code.mc_generate(B, s, seed, si, 0, device=DEV)
        msg = m if msg is None else msg
        ys.append(y)
    return msg, torch.stack(ys).contiguous()


@functools.lru_cache(maxsize=None)
def case_setup(name):
    """(net, decoder, code, cols, msg (B, K), y (n_seg, B, N)) of a case; built once, never written."""
    net_name, precision, reverse, snrs, B = CASES[name]
    if net_name == "pac_128_64":
        import argparse
        from neural_polar_decoder_amd import PAC
        from neural_polar_decoder_amd.montecarlo import seeded_crisp
        code = PAC(argparse.Namespace(target_K=64), 128, 64, 91)
        net, dec = seeded_crisp(code, 64, 2, seed=0, device=DEV, precision=precision)
        cols = np.asarray(code.B)
    else:
        from neural_polar_decoder_amd import reference_polar_code
        from neural_polar_decoder_amd.rnn import RNN_Model, RNN_decoder
        d = trained_fixture(net_name)
        N, F, L = int(d["N"]), int(d["F"]), int(d["layers"])
        net = RNN_Model("GRU", N + 2, F, 1, L, N, 0, 0).to(DEV).eval()
        net.load_state_dict({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w.")})
        dec = RNN_decoder("y_input", N, d["info"], onehot=True, reverse_order=reverse, precision=precision)
        code = reference_polar_code(N, int(d["K"]))
        cols = np.asarray(code.info_positions)
        assert np.array_equal(cols, d["info"])
    msg, y = words(code, snrs, B)
    return net, dec, code, cols, msg, y


@functools.lru_cache(maxsize=None)
def sweep_counts(name):
    """The case's counters from ONE count-only launch (no `decoded`), as an (n_seg, 2) int64 array."""
    net, dec, code, cols, msg, y = case_setup(name)
    c = torch.zeros(y.shape[0], 2, dtype=torch.int64, device=DEV)
    dec.decode_count_sweep(net, y, msg, c, cols=cols)
    return c.cpu().numpy()


def unfused(net, dec, y, msg, cols):
    from neural_polar_decoder_amd.utils import count_errors
    c = torch.zeros(y.shape[0], 2, dtype=torch.int64, device=DEV)
    outs = []
    for s in range(y.shape[0]):
        d = dec.decode(net, False, y[s])
        count_errors(msg, d, c[s], cols=cols)
        outs.append(d)
    return c.cpu().numpy(), torch.stack(outs)


@pytest.mark.parametrize("name", PINNED)
def test_counts_pinned_to_parent(name):
    want = golden("gru_sweep_parent_counts.npz")[name]
    got = sweep_counts(name)
    print(name, got.tolist())
    assert np.array_equal(got, want), (got, want)
    assert int(want[:, 1].sum()) > 0  # not vacuous: the nets make errors on these words


@pytest.mark.parametrize("name", list(CASES))
def test_counts_equal_unfused(name):
    net, dec, code, cols, msg, y = case_setup(name)
    ref, _ = unfused(net, dec, y, msg, cols)
    got = sweep_counts(name)
    assert np.array_equal(got, ref), (got, ref)
    assert int(ref[:, 1].sum()) > 0


@pytest.mark.parametrize("reverse", [False, True])
def test_awkward_cols_and_messages(reverse):
    """cols that omit two information positions (decided and fed back, never compared), list two frozen positions
    (compared against the constant 1.0) and are permuted; messages outside {-1, +1} through the message-code loader."""
    net, dec, code, info, _, y = case_setup("c32_rev" if reverse else "c32_nat")
    y = y[1:3, :2000 + 3].contiguous()
    frozen = np.setdiff1d(np.arange(32), info)
    cols = np.concatenate([np.delete(info, [3, 11]), frozen[[0, 9]]])
    cols = cols[np.random.default_rng(7).permutation(cols.size)]
    assert cols.size == 16 and len(set(cols.tolist())) == 16
    g = torch.Generator(device="cpu").manual_seed(3)
    vals = torch.tensor([-1.0, 1.0, 0.0, 2.0, -3.0, 0.4, -0.6, 1.0, 1.0, -1.0])
    msg = vals[torch.randint(0, len(vals), (y.shape[1], 16), generator=g)].to(DEV)
    ref, dd = unfused(net, dec, y, msg, cols)
    assert bool((dd[:, :, torch.from_numpy(frozen).to(DEV)] == 1.0).all())
    c = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    dec.decode_count_sweep(net, y, msg, c, cols=cols)
    assert np.array_equal(c.cpu().numpy(), ref), (c.cpu().numpy(), ref)
    # the frozen columns' messages are compared: dropping them changes the count
    keep = np.flatnonzero(np.isin(cols, info))
    msg14 = msg[:, torch.from_numpy(keep).to(DEV)].contiguous()
    ref14, _ = unfused(net, dec, y, msg14, cols[keep])
    c14 = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    dec.decode_count_sweep(net, y, msg14, c14, cols=cols[keep])
    assert np.array_equal(c14.cpu().numpy(), ref14)
    assert (ref14[:, 0] < ref[:, 0]).all()


@pytest.mark.parametrize("name", ["c64_rev", "c32_nat", "pac128"])
def test_count_only_equals_general(name):
    """decode_count_sweep with `decoded` runs the general instantiation, without it the count-only one."""
    net, dec, code, cols, msg, y = case_setup(name)
    out = torch.full_like(y, 7.0)
    c = torch.zeros(y.shape[0], 2, dtype=torch.int64, device=DEV)
    dec.decode_count_sweep(net, y, msg, c, cols=cols, decoded=out)
    assert np.array_equal(c.cpu().numpy(), sweep_counts(name))
    ref = torch.stack([dec.decode(net, False, y[s]) for s in range(y.shape[0])])
    assert torch.equal(out, ref)


def test_counters_accumulate():
    net, dec, code, cols, msg, y = case_setup("c64_nat")
    c = torch.zeros(y.shape[0], 2, dtype=torch.int64, device=DEV)
    dec.decode_count_sweep(net, y, msg, c, cols=cols)
    dec.decode_count_sweep(net, y, msg, c, cols=cols)
    assert np.array_equal(c.cpu().numpy(), 2 * sweep_counts("c64_nat"))


# ------------------------------------------------------------------------- more than 64 message columns, K = 256
# name -> (N, K, precision, reverse); K == N: cols is every position, else K random positions, permuted
LONG = {
    "n96_k96": (96, 96, "fp16x3", False),
    "n160_k160": (160, 160, "fp16x3", False),
    "n256_k200": (256, 200, "fp16x3", False),
    "n256_k200_rev": (256, 200, "fp16x3", True),
    "n256_k256": (256, 256, "fp16x3", False),
    "n256_k256_bf16x3": (256, 256, "bf16x3", False),
    "n256_k256_bf16": (256, 256, "bf16", False),
}
LONG_B = 16 * 9 + 5
BOUNDARY_COLUMNS = (63, 64, 127, 128, 191, 192)  # and K - 1


@functools.lru_cache(maxsize=None)
def long_setup(name):
    """(net, decoder, cols, msg (B, K), y (2, B, N)) of a LONG case: a seeded, untrained net (F = 64, 2 layers, one-hot),
    the decoder's information set a seeded random half of the positions (no code is needed), messages +-1 with some
    values outside {-1, +1}; built once, never written."""
    from neural_polar_decoder_amd.rnn import RNN_Model, RNN_decoder
    N, K, precision, reverse = LONG[name]
    rng = np.random.default_rng(1000 + N)
    torch.manual_seed(N)
    net = RNN_Model("GRU", N + 2, 64, 1, 2, N, 0, 0).to(DEV).eval()
    info = np.sort(rng.permutation(N)[:N // 2])
    dec = RNN_decoder("y_input", N, info, onehot=True, reverse_order=reverse, precision=precision)
    cols = np.arange(N) if K == N else rng.permutation(N)[:K]
    g = torch.Generator(device="cpu").manual_seed(3 + N)
    vals = torch.tensor([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, 0.0, 2.0, -3.0, 0.4, -0.6])
    msg = vals[torch.randint(0, len(vals), (LONG_B, K), generator=g)].to(DEV)
    y = (1.0 - 2.0 * (torch.rand(2, LONG_B, N, generator=g) < 0.5).float() + 0.8 * torch.randn(2, LONG_B, N, generator=g))
    return net, dec, cols, msg, y.to(DEV).contiguous()


@pytest.mark.parametrize("name", list(LONG))
def test_message_registers_and_slot_255(name):
    """Exact: the count-only launch == the general instantiation (whose `decoded` is RNN_decoder.decode's) == decode +
    count_errors(cols=...), for the messages as drawn and, for every k in {63, 64, 127, 128, 191, 192, K - 1} below K,
    with column k alone negated -- a column that is skipped, or read from another register, changes the count against
    the unfused one (the negation does change the unfused count: asserted)."""
    from neural_polar_decoder_amd.utils import count_errors
    net, dec, cols, msg, y = long_setup(name)
    K = LONG[name][1]
    dd = torch.stack([dec.decode(net, False, y[s]) for s in range(2)])
    frozen = np.setdiff1d(np.arange(dec.N), dec.info_inds)
    assert bool((dd[:, :, torch.from_numpy(frozen).to(DEV)] == 1.0).all())
    assert 0.05 < float((dd < 0).float().mean()) < 0.5  # the information positions are not decoded to a constant

    def three_ways(m):
        ref = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
        for s in range(2):
            count_errors(m, dd[s], ref[s], cols=cols)
        c = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
        dec.decode_count_sweep(net, y, m, c, cols=cols)
        out = torch.full_like(y, 7.0)
        cg = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
        dec.decode_count_sweep(net, y, m, cg, cols=cols, decoded=out)
        assert torch.equal(out, dd)
        return ref.cpu().numpy(), c.cpu().numpy(), cg.cpu().numpy()

    ref0, c0, cg0 = three_ways(msg)
    print(f"SWEEP {name}: unfused {ref0.tolist()} count-only {c0.tolist()} general {cg0.tolist()}")
    assert np.array_equal(c0, ref0) and np.array_equal(cg0, ref0), (c0, cg0, ref0)
    assert (ref0[:, 0] > 0).all() and (ref0[:, 0] < LONG_B * K).all()
    for k in sorted({k for k in BOUNDARY_COLUMNS + (K - 1,) if k < K}):
        m = msg.clone()
        m[:, k] = -m[:, k]
        ref, c, cg = three_ways(m)
        print(f"SWEEP {name} column {k} negated: unfused {ref.tolist()} count-only {c.tolist()} general {cg.tolist()}")
        assert not np.array_equal(ref, ref0), k
        assert np.array_equal(c, ref) and np.array_equal(cg, ref), (k, c, cg, ref)


@pytest.mark.parametrize("with_decoded", [False, True])
def test_repeat_of_message_255s_position_is_refused(with_decoded):
    """K = 256: a cols that lists the position of message column 255 twice is refused like any other repeat, before
    any launch (the counters stay as they were)."""
    from neural_polar_decoder_amd import _lib
    net, dec, cols, msg, y = long_setup("n256_k256")
    for other in (3, 254):
        bad = cols.copy()
        bad[other] = bad[255]
        c = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
        with pytest.raises(_lib.NpdError, match="repeated column"):
            dec.decode_count_sweep(net, y, msg, c, cols=bad, decoded=torch.empty_like(y) if with_decoded else None)
        assert int(c.abs().sum()) == 0
