"""PAC SC-List decoding without a GPU: the fp32 restatement (tests/pac_scl_ref.py) against the fixtures composed
from the reference's own functions (tests/golden/gen_pac_scl.py), against the reference's pac_sc_decode at L = 1 and
against the reference's Polar SC-List with the identity convolution; and the Python surface.

Bar: bit-exact msg_hat, u_hat and leaf LLRs (every operation is a single fp32 operation in a fixed order)."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from pac_scl_ref import pac_info, pac_scl_ref

PAC_SCL_FIXTURES = ["pac_scl_8_4_L4", "pac_scl_16_8_L2", "pac_scl_32_16_L1", "pac_scl_32_16_L3", "pac_scl_32_16_L4",
                    "pac_scl_32_16_L8", "pac_scl_64_22_L4", "pac_scl_64_32_L8", "pac_scl_128_64_L4",
                    "pac_scl_128_64_L8", "pac_scl_256_128_L4", "pac_scl_256_128_L8"]
SC_PAC_FIXTURES = ["sc_pac_32_16", "sc_pac_64_22", "sc_pac_128_64"]
SCL_SMALL = ["scl_64_32_L4", "scl_32_16_L4", "scl_16_8_L2", "scl_64_32_L8", "scl_32_16_L1", "scl_32_16_L3",
             "scl_8_4_L4"]


def test_fixture_list_is_complete():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "pac_scl_*.npz")))
    assert have == sorted(PAC_SCL_FIXTURES)
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "scl_*.npz")))
    for name in PAC_SCL_FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= largest, name


@pytest.mark.parametrize("name", PAC_SCL_FIXTURES)
def test_restatement_reproduces_fixture(name):
    d = golden(f"{name}.npz")
    assert (d["y"] == 0).any() and (d["u_hat"] == 0).any(), "the crafted zero rows are in the fixture"
    for s in np.unique(d["snr"]):
        m = d["snr"] == s
        leaf, vh, uh = pac_scl_ref(d["y"][m], float(s), d["info"], int(d["g"]), int(d["L"]))
        assert np.array_equal(vh, d["msg_hat"][m]), (name, s)
        assert np.array_equal(uh, d["u_hat"][m]), (name, s)
        assert np.array_equal(leaf, d["leaf"][m]), (name, s)


@pytest.mark.parametrize("name", SC_PAC_FIXTURES)
def test_restatement_l1_is_pac_sc_decode(name):
    """L = 1 against the reference's pac_sc_decode (g = 91), the rows with a zero decision included."""
    d = golden(f"{name}.npz")
    assert (d["u_hat"] == 0).any()
    for s in np.unique(d["snr"]):
        m = d["snr"] == s
        leaf, vh, uh = pac_scl_ref(d["y"][m], float(s), d["info"], 91, 1)
        assert np.array_equal(vh, d["msg_hat"][m]), (name, s)
        assert np.array_equal(uh, d["u_hat"][m]), (name, s)
        assert np.array_equal(leaf, d["leaf"][m]), (name, s)


@pytest.mark.parametrize("name", SCL_SMALL)
def test_restatement_identity_convolution_is_polar_scl(name):
    """g = 2 (g_array = [-1, +1]: no tap, u = v) on a Polar information set against PolarCode.scl_decode's message."""
    d = golden(f"{name}.npz")
    for s in np.unique(d["snr"]):
        m = d["snr"] == s
        _, vh, uh = pac_scl_ref(d["y"][m], float(s), d["info"], 2, int(d["L"]))
        assert np.array_equal(vh, d["msg_hat"][m]), (name, s)
        assert np.array_equal(vh, uh[:, d["info"]])


def test_restatement_rate_profile():
    from neural_polar_decoder_amd import PAC
    for N, K in [(16, 8), (32, 16), (64, 22), (128, 64), (256, 128), (256, 200)]:
        assert np.array_equal(pac_info(N, K), PAC(None, N, K, 91).B)


def test_pac_has_the_list_decoder_surface():
    import inspect
    from neural_polar_decoder_amd import PAC, PolarCode
    for name in ("scl_decode", "pac_scl_decode", "scl_decode_mc"):
        assert callable(getattr(PAC, name, None)), name
    assert list(inspect.signature(PAC.scl_decode).parameters) == list(inspect.signature(PolarCode.scl_decode).parameters)
    assert list(inspect.signature(PAC.scl_decode_mc).parameters) == \
        list(inspect.signature(PolarCode.scl_decode_mc).parameters)
    with pytest.raises(NotImplementedError):
        PAC(None, 32, 16, 53).scl_decode(torch.zeros(4, 32), 1.0, 4, use_CRC=True)


def test_cli_parses_pac_list_size():
    from neural_polar_decoder_amd import montecarlo
    a = montecarlo._parse_args(["--code", "pac", "--list_size", "4"])
    assert a.code == "pac" and a.list_size == 4
    assert "PAC" in montecarlo.SCLMonteCarlo.__doc__


def test_no_cpu_fallback():
    """Host inputs are staged to the GPU: with no GPU visible the call raises; with one, it computes there and
    returns host tensors."""
    from neural_polar_decoder_amd import PAC, NpdError
    pac = PAC(None, 32, 16, 53)
    if not torch.cuda.is_available():
        with pytest.raises(NpdError):
            pac.scl_decode(torch.zeros(4, 32), 1.0, 4)
        with pytest.raises(NpdError):
            pac.pac_scl_decode(torch.zeros(4, 32), 1.0, 4)
        with pytest.raises(NpdError):
            pac.scl_decode_mc(torch.zeros(4, 32), 1.0, 4, 1, 0, torch.zeros(2, dtype=torch.int64))
    else:
        llr, hat = pac.scl_decode(torch.zeros(4, 32), 1.0, 4)
        assert not hat.is_cuda and hat.shape == (4, 16) and llr.shape == (4, 32) and bool((hat == 0).all())
