"""The count-only sweep with two codeword tiles per wave (gru16p_kernel<SPLIT, true, 2>: a wave owns tiles 2p and 2p + 1
of one segment and feeds both from each weight fragment it reads): the counters are exactly the unfused sequence's.

Reference: per segment RNN_decoder.decode (the general instantiation, one tile per wave) + count_errors on the same
words.  The words of a case are drawn once at B = 83 and decoded once per segment; a smaller B is their first B rows
(codewords decode independently), so the reference of every size comes from that one decode.

Sizes B = 1, 15, 16, 17, 31, 32, 33, 47, 48, 83 with 1 and 3 segments: a lone first tile (1, 15, 16), a ragged second
tile (17, 31), a full pair (32), an absent second tile behind a full pair (33, 47, 48: three tiles per segment, the
last pair's second tile has no valid lane), six tiles with a ragged last (83); with 3 segments every wave flushes its
counters at a segment change.  All bars exact (integer counters)."""
import functools

import numpy as np
import pytest
import torch

from conftest import trained_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIZES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 83)
SNRS = (-1.0, 0.0, 1.0)
# name -> (net, precision, reverse)
CASES = {
    "c32_fp16x3": ("trained_crisp_32_16", "fp16x3", False),
    "c32_bf16x3": ("trained_crisp_32_16", "bf16x3", False),
    "c32_bf16": ("trained_crisp_32_16", "bf16", False),
    "c64_nat": ("trained_crisp_64_32", "fp16x3", False),
    "c64_rev": ("trained_crisp_64_32", "fp16x3", True),
}


@functools.lru_cache(maxsize=None)
def case_setup(name):
    """(net, decoder, cols, msg (83, K), y (3, 83, N), decisions (3, 83, N)) of a case; built once, never written."""
    from neural_polar_decoder_amd import reference_polar_code
    from neural_polar_decoder_amd.rnn import RNN_Model, RNN_decoder
    net_name, precision, reverse = CASES[name]
    d = trained_fixture(net_name)
    N, F, L = int(d["N"]), int(d["F"]), int(d["layers"])
    net = RNN_Model("GRU", N + 2, F, 1, L, N, 0, 0).to(DEV).eval()
    net.load_state_dict({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w.")})
    dec = RNN_decoder("y_input", N, d["info"], onehot=True, reverse_order=reverse, precision=precision)
    code = reference_polar_code(N, int(d["K"]))
    cols = np.asarray(code.info_positions)
    ys, msg = [], None
    for si, s in enumerate(SNRS):
        m, _, y = code.mc_generate(max(SIZES), s, 23, si, 0, device=DEV)
        msg = m if msg is None else msg
        ys.append(y)
    y = torch.stack(ys).contiguous()
    dd = torch.stack([dec.decode(net, False, y[s]) for s in range(len(SNRS))])
    return net, dec, cols, msg, y, dd


@pytest.mark.parametrize("name", list(CASES))
def test_pair_counts_equal_unfused(name):
    from neural_polar_decoder_amd.utils import count_errors
    net, dec, cols, msg, y, dd = case_setup(name)
    block_errors = 0
    for nseg in (1, 3):
        for B in SIZES:
            m = msg[:B].contiguous()
            ref = torch.zeros(nseg, 2, dtype=torch.int64, device=DEV)
            for s in range(nseg):
                count_errors(m, dd[s, :B].contiguous(), ref[s], cols=cols)
            c = torch.zeros(nseg, 2, dtype=torch.int64, device=DEV)
            dec.decode_count_sweep(net, y[:nseg, :B].contiguous(), m, c, cols=cols)
            got, want = c.cpu().numpy(), ref.cpu().numpy()
            print(f"PAIR {name} nseg {nseg} B {B}: count-only {got.tolist()} unfused {want.tolist()}")
            assert np.array_equal(got, want), (name, nseg, B, got, want)
            assert (want[:, 1] <= B).all() and (want[:, 0] <= B * cols.size).all()
            block_errors += int(want[:, 1].sum())
    assert block_errors > 0  # not vacuous: the net makes block errors on these words


def test_slices_decode_as_the_whole():
    """The shared reference rests on codewords decoding independently of their batch: the first 17 rows decoded alone
    are the first 17 rows of the 83-row decode."""
    net, dec, cols, msg, y, dd = case_setup("c32_fp16x3")
    assert torch.equal(dec.decode(net, False, y[1, :17].contiguous()), dd[1, :17])
