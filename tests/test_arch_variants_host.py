"""CPU halves of tests/test_arch_variants.py: the oracle against the fixtures of the four architectures off the shipped two
(tests/golden/arch_<name>.npz, written from the real reference by tests/golden/make_golden_archs.py), the YAML round trip of
each, and the acceptance boundary: an architecture the library has no kernels for is refused when the model is created, by
wt_model_create before any HIP call and by wt_packed_info on a header, with a message that names the field."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from tests import arch_ref as A
from tests.util import NEAR_TIE_MARGIN, check_codes, rel_l2

FLOAT_TOL = 2e-5          # tests/test_oracle_golden.py: bit-identical where the fixture was written, oneDNN's choice elsewhere


@pytest.mark.parametrize("case", A.CASES)
@pytest.mark.parametrize("name", A.VARIANTS)
def test_oracle_reproduces_the_fixture(name, case):
    torch.set_num_threads(8)
    arch, cases, g = A.variant(name)
    B, T, _seed, _bw = cases[case]
    L = arch.frames(T)
    r = A.oracle_run(name, case)
    assert r["codes"].dtype == torch.int64 and tuple(r["codes"].shape) == g[f"{case}/codes"].shape == (1, B, L)
    assert float(g[f"{case}/margin"].min()) > NEAR_TIE_MARGIN           # no frame of a fixture is excused as a near tie
    assert check_codes(r["codes"].numpy(), g[f"{case}/codes"], g[f"{case}/margin"], f"{name}/{case}") == 0
    wav = r["wav"].numpy()
    assert wav.shape == (B, L * arch.hop_length)
    want = g[f"{case}/wav_out"]
    assert rel_l2(wav[:want.shape[0]], want) < FLOAT_TOL
    l2 = np.sqrt((wav.astype(np.float64) ** 2).sum(axis=1))
    assert np.allclose(l2, g[f"{case}/wav_out_l2"], rtol=FLOAT_TOL, atol=0)
    H = int(g["head_steps"])
    stages = [k.split("/")[2] for k in g.files if k.startswith(f"{case}/tap/") and k.endswith("/l2")]
    assert set(stages) == set(r["taps"]) - {"vq.margin"}
    for st in stages:
        a = r["taps"][st].numpy()
        assert tuple(g[f"{case}/tap/{st}/shape"]) == a.shape, st
        want_l2 = float(g[f"{case}/tap/{st}/l2"])
        assert abs(np.sqrt((a.astype(np.float64) ** 2).sum()) - want_l2) <= FLOAT_TOL * want_l2, st
        head = a[0, :H] if st == "bb.out" else a[0, :, :H]
        assert rel_l2(head, g[f"{case}/tap/{st}/head"]) < 5 * FLOAT_TOL, st


@pytest.mark.parametrize("name", A.VARIANTS)
def test_yaml_round_trip_and_what_the_variant_reaches(name):
    from wavtokenizer_amd.config import arch_from_yaml_dict
    arch, cases, _g = A.variant(name)
    assert arch_from_yaml_dict({"model": {"init_args": arch.to_yaml_node()}}) == arch
    # the cases are the ones the shapes were chosen for: 6 frames with a ragged last hop; 130 frames x 8 clips
    assert cases["small"][:2] == (2, 5 * arch.hop + 17) and cases["rows"][:2] == (8, 129 * arch.hop + 1)
    assert cases["small"][3] == arch.adanorm_num_embeddings - 1 and cases["rows"][3] == 0
    assert arch.hop == arch.hop_length
    reach = {"narrow": (3, 256, 96, 8, 2), "mid16": (5, 512, 1504, 1024, 6),
             "last16": (16, 256, 96, 8, 2), "wide": (2, 1024, 2080, 16384, 4)}[name]
    assert (arch.enc_ratios[0], arch.dim, arch.intermediate_dim, arch.vq_bins, arch.n_fft // arch.hop_length) == reach
    if name == "mid16":
        assert 2 * max(arch.ratios) == 32 and (arch.intermediate_dim // 32) % 2 == 1 and arch.vq_bins % 192       # the most taps a GEMM gathers
        assert -(-(arch.n_fft // 4 + 1) // 32) * 32 == 736


def _wt_arch(arch):
    from wavtokenizer_amd import _capi
    wa = _capi.WtArch()
    wa.n_ratios = len(arch.ratios)
    for i, r in enumerate(arch.ratios):
        wa.ratios[i] = r
    wa.vq_bins, wa.num_quantizers, wa.input_channels = arch.vq_bins, arch.num_quantizers, arch.input_channels
    wa.dim, wa.intermediate_dim, wa.num_layers = arch.dim, arch.intermediate_dim, arch.num_layers
    wa.adanorm_num_embeddings, wa.n_fft, wa.hop_length = arch.adanorm_num_embeddings, arch.n_fft, arch.hop_length
    wa.padding_same = 1 if arch.padding == "same" else 0
    return wa


def _create(arch):
    """wt_model_create with one empty tensor record: whatever is decided on the architecture alone is decided before it."""
    from wavtokenizer_amd import _capi
    out = ctypes.c_void_p()
    t = (_capi.WtTensor * 1)()
    rc = _capi.lib.wt_model_create(ctypes.byref(_wt_arch(arch)), t, 0, 0, ctypes.byref(out))
    msg = _capi.lib.wt_last_error().decode()
    if out.value:
        _capi.lib.wt_model_destroy(out)
    return rc, msg, out.value


def _packed_info(arch):
    from wavtokenizer_amd import _capi
    from tests.test_host_logic import _packed_header
    buf = _packed_header(arch)
    rc = _capi.lib.wt_packed_info(buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, None, None, None)
    return rc, _capi.lib.wt_last_error().decode()


# field changes on hop600 -> the text of the refusal.  All of them are made by wt_model_create before any HIP call (so they come
# back as WT_ERR_INVALID on a host without a GPU, where the first HIP call would give WT_ERR_HIP) and by wt_packed_info
REFUSALS = [
    (dict(dim=1280), "dim must be 256, 512, 768 or 1024"),              # % 256 == 0, but no row kernel: failed at a launch before
    (dict(dim=128), "dim must be 256, 512, 768 or 1024"),
    (dict(dim=0), "dim must be 256, 512, 768 or 1024"),
    (dict(intermediate_dim=100), "intermediate_dim must be a positive multiple of 32"),
    (dict(intermediate_dim=0), "intermediate_dim must be a positive multiple of 32"),
    (dict(vq_bins=6), "vq_bins must be a positive multiple of 4"),
    (dict(adanorm_num_embeddings=0), "adanorm_num_embeddings must be >= 1"),
    (dict(ratios=(6, 5, 5)), "ratios: the encoder width after the last ratio must be 512"),      # three ratios: width 256
    (dict(ratios=(6, 5, 5, 4, 2)), "ratios: the encoder width after the last ratio must be 512"),
    (dict(ratios=(17, 5, 5, 4)), "ratios: every ratio must be 1 .. 16"),      # 34 taps: loaded, then failed at the conv's launch
    (dict(ratios=(6, 0, 5, 4)), "ratios: every ratio must be 1 .. 16"),
    # the variant first planned as `mid`: its down conv of 40 taps is beyond both GEMM engines (32), so its class is refused
    (dict(ratios=(20, 3, 2, 4), vq_bins=1024, dim=512, intermediate_dim=1504, num_layers=3, n_fft=2880, hop_length=480),
     "ratios: every ratio must be 1 .. 16"),
    (dict(n_fft=225, hop_length=75), "n_fft must be an even multiple of hop_length"),             # 3 x an odd hop_length
    (dict(n_fft=2400, hop_length=700), "n_fft must be an even multiple of hop_length"),
    (dict(n_fft=1206, hop_length=402), "n_fft % 4 must be 0"),
    (dict(n_fft=2400, hop_length=0), "hop_length >= 1"),
    (dict(input_channels=256), "input_channels must be 512"),
    (dict(num_quantizers=33), "num_quantizers must be 1 .. 32"),
    (dict(num_quantizers=0), "num_quantizers must be 1 .. 32"),
    (dict(num_layers=33), "num_layers must be 1 .. 32"),                # was refused at plan creation only (the range sites)
    (dict(num_layers=0), "num_layers must be 1 .. 32"),
]


@pytest.mark.parametrize("change,text", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in list(c.items())[:2]) for c, _ in REFUSALS])
def test_refused_when_the_model_is_created(change, text):
    from wavtokenizer_amd import _capi, NAMED_ARCHS
    arch = dataclasses.replace(NAMED_ARCHS["hop600"], **change)
    rc, msg, model = _create(arch)
    assert rc == _capi.WT_ERR_INVALID and text in msg and not model, (rc, msg)
    rc, msg = _packed_info(arch)
    assert rc == _capi.WT_ERR_INVALID and text in msg and msg.startswith("packed image: "), (rc, msg)


@pytest.mark.parametrize("name", A.VARIANTS + ("hop600", "hop320"))
def test_architectures_that_run_pass_the_rule(name):
    """The control of the table above: the variants (and the shipped two) pass the architecture rule; with no tensors the
    creation then ends at the first HIP call (no GPU) or at the first missing tensor, never as WT_ERR_INVALID."""
    from wavtokenizer_amd import _capi, NAMED_ARCHS
    arch = NAMED_ARCHS[name] if name in NAMED_ARCHS else A.variant(name)[0]
    rc, msg, model = _create(arch)
    assert rc not in (0, _capi.WT_ERR_INVALID) and not model, (rc, msg)
    assert _packed_info(arch)[0] == 0
