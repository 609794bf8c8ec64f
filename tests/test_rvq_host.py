"""The host side of residual VQ encode without a GPU: the constants and entry points on both sides of the C ABI, the CPU
reference of tests/rvq_ref.py against the fixture captured from the reference (tests/golden/hop600_rvq3.npz), the bandwidth ->
K arithmetic, and the argument errors that must be raised before any GPU work."""
import ctypes
import dataclasses
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import rvq_ref as R
from tests import vq_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "hop600_rvq3.npz")
TAGS = (("all", None, 3), ("bw0p6", 0.6, 2), ("bw0p1", 0.1, 1))


@pytest.fixture(scope="module")
def gold():
    from wavtokenizer_amd import ARCH_HOP600, synth
    g = np.load(GOLD)
    arch = dataclasses.replace(ARCH_HOP600, num_quantizers=3)
    sd = synth.make_state_dict(arch, seed=int(g["weight_seed"]))
    books = [torch.from_numpy(sd["feature_extractor.encodec.quantizer.vq.layers.%d._codebook.embed" % k]) for k in range(3)]
    return g, arch, books


def test_header_and_capi_constants_agree():
    from wavtokenizer_amd import _capi          # (binds the built library: the entry points must be exported)
    with open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")) as f:
        h = f.read()

    def const(name):
        return int(re.search(r"\b%s\s*=\s*(\d+)" % name, h).group(1))

    assert const("WT_PLAN_QUANTIZE") == _capi.WT_PLAN_QUANTIZE == 8
    assert const("WT_PLAN_FLAG_RVQ") == _capi.WT_PLAN_FLAG_RVQ == 256
    flags = [const(n) for n in re.findall(r"\b(WT_PLAN_FLAG_\w+)\s*=\s*\d+", h)]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags), "plan flags are distinct single bits"


def test_new_exports_have_signatures():
    from wavtokenizer_amd import _capi
    with open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")) as f:
        h = f.read()
    for name, nargs in (("wt_encode_rvq", 6), ("wt_encode_rvq_mixed", 7), ("wt_quantize", 6), ("wt_vq_residual_probe", 3),
                        ("wt_model_codebook_tables", 5)):
        assert name in _capi.EXPORTS and re.search(r"\bint %s\(" % name, h), name
        fn = getattr(_capi.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    # the probe descriptor as the header lays it out: four int32, rows on 8 bytes, nine pointers
    assert [n for n, _t in _capi.WtVqResidualDesc._fields_] == ["size", "D", "bins", "nparts", "rows", "pval", "pidx", "x", "embed", "codes",
                                                                "r", "r_s32", "xx", "status"]
    assert ctypes.sizeof(_capi.WtVqResidualDesc) == 16 + 8 + 9 * 8 and _capi.WtVqResidualDesc.rows.offset == 16
    for doc in ("Replaces: SEANetEncoder", "Replaces: ResidualVectorQuantizer.encode"):
        assert doc in h


def test_probe_refuses_descriptors_before_any_hip_call():
    """D % 256, a null pointer, nparts < 1, a wrong size, misaligned arrays: WT_ERR_INVALID with a message; the pointers are not
    even valid, so a launch would fault."""
    from wavtokenizer_amd import _capi
    fake = 1 << 20

    def rc(**kw):
        d = _capi.WtVqResidualDesc()
        d.size = ctypes.sizeof(d)
        d.D, d.bins, d.nparts, d.rows = 512, 100, 2, 5
        for i, n in enumerate(("pval", "pidx", "x", "embed", "codes", "r", "r_s32", "xx", "status")):
            setattr(d, n, (i + 1) * fake)
        for k, v in kw.items():
            setattr(d, k, v)
        return _capi.lib.wt_vq_residual_probe(ctypes.byref(d), None, None), _capi.lib.wt_last_error().decode()

    for kw, msg in ((dict(D=384), "multiple of 256"), (dict(D=0), "D >= 1"), (dict(nparts=0), "nparts >= 1"), (dict(rows=0), "rows"),
                    (dict(bins=0), "bins >= 1"), (dict(size=8), "another size"), (dict(x=None), "required"), (dict(pval=None), "required"),
                    (dict(pidx=None), "required"), (dict(embed=None), "required"), (dict(codes=None), "required"), (dict(r=None), "required"),
                    (dict(xx=None), "required"), (dict(r=fake + 4), "16-byte"), (dict(r_s32=fake + 8), "16-byte"),
                    (dict(codes=fake + 4), "8-byte"), (dict(status=fake + 2), "4-byte")):
        code, err = rc(**kw)
        assert code == _capi.WT_ERR_INVALID and msg in err, (kw, err)


@pytest.mark.parametrize("tag,bandwidth,K", TAGS)
def test_cpu_reference_reproduces_the_fixture(gold, tag, bandwidth, K):
    g, arch, books = gold
    emb = torch.from_numpy(g["emb"])
    assert tuple(emb.shape) == (2, 512, 40) and int(g[f"{tag}/K"]) == K
    assert R.num_quantizers_for_bandwidth(arch.vq_bins, 3, int(g["frame_rate"]), bandwidth) == K
    want = torch.from_numpy(g[f"{tag}/codes"])
    assert tuple(want.shape) == (K, 2, 40) and want.dtype == torch.int64
    assert torch.equal(R.encode(emb, books, K), want)


def test_prefix_property_on_the_fixture(gold):
    g, _arch, _books = gold
    full = g["all/codes"]
    assert np.array_equal(g["bw0p6/codes"], full[:2]) and np.array_equal(g["bw0p1/codes"], full[:1])
    assert all(len(np.unique(full[k])) > 20 for k in range(3)), "the fixture's codes are spread over the codebooks"


def test_fixture_leaves_out_at_most_two_percent(gold):
    """The condition the generator asserts, on the stored data: with either distance kernel's bound and the model's own |e|^2
    tables, at most 2 % of the reference's frames are undecidable in any round."""
    g, _arch, books = gold
    rows = R.rows_of(torch.from_numpy(g["emb"]))
    ees = [V.host_serial_ee(e) for e in books]
    for kernel in (0, 1):
        und = R.undecidable_rows(rows, books, torch.from_numpy(g["all/codes"]).reshape(3, -1), kernel, ees)
        assert int(und.any(0).sum()) <= 0.02 * rows.shape[0], (kernel, und.sum(1).tolist())


def test_teacher_forced_checker_accepts_the_reference_and_rejects_a_wrong_code(gold):
    g, _arch, books = gold
    rows = R.rows_of(torch.from_numpy(g["emb"]))
    ees = [V.host_serial_ee(e) for e in books]
    codes = torch.from_numpy(g["all/codes"]).reshape(3, -1).clone()
    for kernel in (0, 1):
        res = R.check_teacher_forced(codes, rows, books, kernel, ees)
        assert all(ok == rows.shape[0] and strict >= 0.95 * ok for strict, ok in res)
        assert R.check_against(codes, codes, rows, books, kernel, ees) <= 2
    bad = codes.clone()
    bad[1, 7] = (bad[1, 7] + 1) % books[1].shape[0]          # a wrong code in round 1: round 1 fails (round 2 is then teacher-forced on it)
    with pytest.raises(AssertionError, match="round 1"):
        R.check_teacher_forced(bad, rows, books, 1, ees)
    with pytest.raises(AssertionError, match="differ from the fixture"):
        R.check_against(bad, codes, rows, books, 1, ees)
    # a residual that was not subtracted in fp32 from the chosen row shows in the next round: codes of round 1 chosen on r_0
    lazy = codes.clone()
    lazy[1] = R.nearest(rows, books[1])
    with pytest.raises(AssertionError, match="round 1"):
        R.check_teacher_forced(lazy, rows, books, 1, ees)


def test_bandwidth_arithmetic_matches_the_reference():
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(dataclasses.replace(ARCH_HOP600, num_quantizers=3))
    q = m.feature_extractor.encodec.quantizer
    fr = m.feature_extractor.frame_rate
    assert fr == 25 and q.bins == 4096 and q.n_q == 3
    assert q.get_bandwidth_per_quantizer(fr) == math.log2(4096) * 25 == 300.0
    # vq.py:142-151: None, 0 and negative give every layer; otherwise max(1, floor(bandwidth * 1000 / 300)), not cut here ...
    for bandwidth, n_q in ((None, 3), (0, 3), (0.0, 3), (-1.5, 3), (0.1, 1), (0.29, 1), (0.3, 1), (0.6, 2), (0.9, 3), (6.6, 22), (100.0, 333)):
        assert q.get_num_quantizers_for_bandwidth(fr, bandwidth) == n_q, bandwidth
        # ... and cut to the number of layers by encode (core_vq.py:407): K of the codes
        assert R.num_quantizers_for_bandwidth(q.bins, q.n_q, fr, bandwidth) == min(n_q, 3), bandwidth
    m1 = WavTokenizer.from_arch(ARCH_HOP600)
    assert m1.feature_extractor.encodec.quantizer.get_num_quantizers_for_bandwidth(25, 6.6) == 22
    assert m1.feature_extractor.encodec.quantizer.get_num_quantizers_for_bandwidth(25, None) == 1


def test_argument_errors_are_raised_before_any_gpu_work():
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    from wavtokenizer_amd._capi import WavTokError
    m = WavTokenizer.from_arch(dataclasses.replace(ARCH_HOP600, num_quantizers=3))     # on the CPU, no engine: any real call raises RuntimeError
    wav = torch.zeros(1, 2400)
    for bad in (0, 4, -1):
        with pytest.raises(WavTokError, match="n_q must be between 1 and the number of codebooks"):
            m.encode_codes(wav, n_q=bad)
        with pytest.raises(WavTokError, match="n_q must be between 1 and the number of codebooks"):
            m.encode_codes_many([wav[0]], n_q=bad)
    for bad in (1.5, "2", True, torch.tensor(2)):
        with pytest.raises(ValueError, match="n_q must be an int"):
            m.encode_codes(wav, n_q=bad)
        with pytest.raises(ValueError, match="n_q must be an int"):
            m.encode_codes_many([wav[0]], n_q=bad)
    with pytest.raises(ValueError):
        m.encode_codes_many([torch.zeros(2, 3, 4)], n_q=2)                               # the clip checks still come first
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        m.encode_codes(wav, n_q=3)                                                       # a valid call reaches the engine
    q = m.feature_extractor.encodec.quantizer
    for bad in (torch.zeros(2, 512), torch.zeros(1, 256, 5), torch.zeros(1, 5, 512), [[0.0]]):
        with pytest.raises(ValueError, match="codebook width"):
            q.encode(bad, 25)
    with pytest.raises(ValueError, match="empty"):
        q.encode(torch.zeros(1, 512, 0), 25)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        q.encode(torch.zeros(1, 512, 5), 25, 0.6)


def test_encode_codes_many_threads_n_q_to_every_group_and_keeps_todays_calls_without_it():
    """Over recording stubs on a model that was never loaded: with n_q the flat tensor is [n_q][sum L_i] and every group and the
    solo remainder are sent n_q; without it the stubs are called with today's arguments, no more."""
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(dataclasses.replace(ARCH_HOP600, num_quantizers=3))
    seen = []

    def mixed(part, T_pad, flat, offs, *rest):
        seen.append(("mixed", len(part), tuple(flat.shape), rest))
        for sp, off in zip(part, offs):
            flat[..., off:off + m.arch.frames(sp.n_out)] = len(part)
        return True

    def solo(part, flat, offs, *rest):
        seen.append(("solo", len(part), tuple(flat.shape), rest))
        for sp, off in zip(part, offs):
            flat[..., off:off + m.arch.frames(sp.n_out)] = 1

    m._run_encode_codes_mixed, m._encode_codes_solo = mixed, solo
    clips = [torch.zeros(n) for n in (9000, 9100, 700, 24000, 23000)]
    frames = [m.arch.frames(n) for n in (9000, 9100, 700, 24000, 23000)]
    out = m.encode_codes_many(clips, n_q=2)
    assert [tuple(o.shape) for o in out] == [(2, 1, L) for L in frames]
    assert all(shape == (2, sum(frames)) and rest == (2,) for _w, _n, shape, rest in seen) and {w for w, *_r in seen} == {"mixed", "solo"}
    assert sorted(n for _w, n, *_r in seen) == [1, 2, 2]
    flat, offs = m.encode_codes_many(clips, n_q=3, packed=True)
    assert tuple(flat.shape) == (3, sum(frames)) and offs.tolist() == np.concatenate([[0], np.cumsum(frames)]).tolist()
    assert bool((flat > 0).all()), "every clip's span of every plane was written"
    seen.clear()
    out = m.encode_codes_many(clips)
    assert [tuple(o.shape) for o in out] == [(1, 1, L) for L in frames]
    assert all(shape == (sum(frames),) and rest == () for _w, _n, shape, rest in seen) and len(seen) == 3
