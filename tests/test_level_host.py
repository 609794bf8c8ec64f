"""Per-clip level control without a GPU: the argument errors of the new arguments (raised before any GPU work: the model here
lives on the CPU, where any GPU work would raise RuntimeError instead), SegmentedCodes with and without scales, the new exports
against the header, and tests/level_ref.py against the reference's three expressions, restated here."""
import os
import re

import numpy as np
import pytest
import torch

from tests import level_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"wt_level_chunk": 0, "wt_level_workspace_bytes": 2, "wt_level": 4, "wt_normalize_rows_workspace_bytes": 2,
               "wt_normalize_rows": 9, "wt_scale_rows": 6, "wt_emit_rescaled_workspace_bytes": 1, "wt_emit_rescaled": 4}


@pytest.fixture(scope="module")
def model():
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    return WavTokenizer.from_arch(ARCH_HOP600)                 # on the CPU: nothing here may reach the GPU


def test_normalize_arguments_raise_before_any_gpu_work(model):
    wav = torch.zeros(1, 2400)
    clips = [torch.zeros(2400)]
    calls = {
        "encode_codes": lambda **kw: model.encode_codes(wav, **kw),
        "encode_codes_many": lambda **kw: model.encode_codes_many(clips, **kw),
        "encode_codes_segmented": lambda **kw: model.encode_codes_segmented(clips[0], 1200, 600, **kw),
        "encode_codes_segmented_many": lambda **kw: model.encode_codes_segmented_many(clips, 1200, 600, **kw),
    }
    for name, call in calls.items():
        for kw in (dict(target_db=-3.0), dict(normalize="rms", target_db=-3.0), dict(normalize="loudness"), dict(normalize="PEAK"),
                   dict(normalize="peak", target_db=float("nan")), dict(normalize="peak", target_db="3")):
            with pytest.raises(ValueError):
                call(**kw)
        if "segmented" not in name:
            with pytest.raises(ValueError, match="return_scales"):
                call(return_scales=True)
        with pytest.raises(RuntimeError):                      # the arguments are fine: the next thing is the GPU
            call(normalize="peak", target_db=-3.0)


def test_scales_and_rescale_arguments(model):
    codes = torch.zeros((1, 2, 4), dtype=torch.int64)
    for bad in (torch.ones(3), torch.ones(2, 1), torch.ones(2, dtype=torch.int64), [1.0, 1.0]):
        with pytest.raises(ValueError, match="scales"):
            model.decode_pcm(codes, bandwidth_id=0, scales=bad)
        with pytest.raises(ValueError, match="scales"):
            model.decode_pcm_many([codes[:, 0], codes[:, 1]], bandwidth_id=0, scales=bad)
    with pytest.raises(ValueError, match="limit"):            # the limit is checked with rescale as without it, for fp32 too
        model.decode_pcm(codes, bandwidth_id=0, rescale=True, dtype=torch.float32, limit=1.5)
    with pytest.raises(RuntimeError):
        model.decode_pcm(codes, bandwidth_id=0, rescale=True, scales=torch.ones(2))


def test_audio_normalize_and_level_arguments():
    from wavtokenizer_amd import audio
    x = torch.zeros(2, 100)
    for kw in (dict(mode="loudness"), dict(mode=None), dict(mode="rms", target_db=-3.0), dict(mode="peak", target_db=float("inf"))):
        with pytest.raises(ValueError):
            audio.normalize(x, **kw)
    for bad in (torch.zeros(2, 2, 100), torch.zeros(0), torch.zeros(2, 3, 4, 5), [0.0]):
        with pytest.raises(ValueError):
            audio.normalize(bad)
    with pytest.raises(RuntimeError, match="GPU only"):        # there is no CPU path
        audio.normalize(x)
    for bad in ([], [torch.zeros(0)], [torch.zeros(2, 3)], [torch.zeros(4, dtype=torch.float64)]):
        with pytest.raises(ValueError):
            audio.level_many(bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        audio.level(torch.zeros(10))
    assert audio.normalize_args("f", None, 0.0) is None
    assert audio.normalize_args("f", "rms", 0) == (1, 1.0) and audio.normalize_args("f", "peak", 0.0) == (0, 1.0)
    mode, gain = audio.normalize_args("f", "peak", -3.0)
    assert mode == 0 and gain == float(np.float32(10.0 ** (-3.0 / 20.0))) == R.gain_of(-3.0) and gain != 10.0 ** (-3.0 / 20.0)


def test_segmented_codes_with_and_without_scales():
    from wavtokenizer_amd import ARCH_HOP600
    from wavtokenizer_amd.segmented import SegmentedCodes
    codes = torch.arange(10, dtype=torch.int64)                # 3000 samples in segments of 2400, stride 1200: 4 + 3 + 1 ... frames
    frames = [ARCH_HOP600.frames(n) for n in (2400, 1800, 600)]
    assert frames == [4, 3, 1]
    offsets = [0, 4, 7, 8]
    plain = SegmentedCodes(codes[:8], offsets, 3000, 2400, 1200)
    assert plain.scales is None and "scales" not in repr(plain)
    plain.validate(ARCH_HOP600)
    scales = torch.tensor([0.5, 0.25, 0.125])
    with_scales = SegmentedCodes(codes[:8], offsets, 3000, 2400, 1200, scales)
    assert with_scales.scales is scales and "scales=(3,) on cpu" in repr(with_scales)
    assert repr(with_scales).startswith(repr(plain)[:-1])
    with_scales.validate(ARCH_HOP600)
    with pytest.raises(ValueError, match="scales"):
        SegmentedCodes(codes[:8], offsets, 3000, 2400, 1200, torch.ones(2)).validate(ARCH_HOP600)
    for bad in (torch.ones(3, 1), torch.ones(3, dtype=torch.int64), [0.5, 0.25, 0.125]):
        with pytest.raises(ValueError, match="scales"):
            SegmentedCodes(codes[:8], offsets, 3000, 2400, 1200, bad)
    segs = [codes[0:4], codes[4:7].view(1, 3), codes[7:8].view(1, 1, 1)]
    a = SegmentedCodes.from_segments(segs, 3000, 2400, 1200)
    assert a.scales is None and a.offsets.tolist() == offsets
    b = SegmentedCodes.from_segments(segs, 3000, 2400, 1200, scales)
    assert b.scales is scales
    c = SegmentedCodes.from_segments(segs, 3000, 2400, 1200, [scales[0:1], scales[1].reshape(1, 1), scales[2]])
    d = SegmentedCodes.from_segments(segs, 3000, 2400, 1200, [0.5, 0.25, 0.125])
    for sc in (b, c, d):
        assert sc.scales.dtype == torch.float32 and torch.equal(sc.scales, scales) and torch.equal(sc.codes, codes[:8])
        sc.validate(ARCH_HOP600)


def test_new_exports_match_the_header():
    from wavtokenizer_amd import _capi
    header = open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")).read()
    for name, n_args in NEW_EXPORTS.items():
        m = re.search(r"^(size_t|int|int32_t)\s+%s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        args = [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
        assert len(args) == n_args, (name, args)
        assert name in _capi.EXPORTS
        fn = getattr(_capi.lib, name)
        assert len(fn.argtypes) == n_args, name
        if m.group(1) == "size_t":
            assert fn.restype is _capi.c_size_t, name
    assert re.search(r"int\s+wt_level\(const wt_level_clip\* clips, int32_t B, void\* workspace, void\* stream\);", header)
    assert re.search(r"int\s+wt_emit_rescaled\(const wt_emit_clip\* clips, int32_t B, void\* workspace, void\* stream\);", header)
    assert "WT_NORM_PEAK = 0, WT_NORM_RMS = 1" in header and (_capi.WT_NORM_PEAK, _capi.WT_NORM_RMS) == (0, 1)
    assert "is not offered: take fp32 out" not in header       # wt_emit's comment no longer says rescale is missing
    assert int(_capi.lib.wt_level_chunk()) == 4096
    assert int(_capi.lib.wt_level_workspace_bytes(0, 10)) == 0 and int(_capi.lib.wt_emit_rescaled_workspace_bytes(0)) == 0
    assert int(_capi.lib.wt_emit_rescaled_workspace_bytes(3)) == int(_capi.lib.wt_emit_workspace_bytes(3)) + 12
    # every clip's chunks fit: B clips of 1 sample need B partials of each kind
    assert int(_capi.lib.wt_level_workspace_bytes(70, 70)) >= 70 * 32 + 3 * 4 * 70


def test_level_ref_is_the_references_three_expressions():
    rng = np.random.default_rng(3)
    for n in (1, 7, 1000, 30011):
        wav = torch.from_numpy((rng.standard_normal((1, n)) * 0.2).astype(np.float32))         # [1, T] as convert_audio returns it
        # extract_features.py:27-28
        want = wav / (wav.abs().max() + 1e-8)
        got, scale = R.peak_normalize(wav[0])
        assert torch.equal(got, want[0]) and float(scale) == float(wav.abs().max() + 1e-8)
        # encoder/model.py:153-156 on x [B, C, T] with one channel
        x = wav[None]
        mono = x.mean(dim=1, keepdim=True)
        volume = mono.pow(2).mean(dim=2, keepdim=True).sqrt()
        ref_scale = 1e-8 + volume
        got, scale = R.rms_normalize(wav[0])
        assert torch.equal(got, (x / ref_scale)[0, 0]) and float(scale) == float(ref_scale)
        assert abs(float(scale) - (1e-8 + R.rms64(wav[0].numpy()))) <= R.rms_bound(n) * float(scale)
        # encoder/utils.py:95-103 with rescale=True.  torch evaluates `limit / mx` (a Python number over a tensor) as
        # mx.reciprocal() * limit, two roundings where the library's one division (wt_pcm16's rule, kept by wt_emit_rescaled) has
        # one: the factors agree within 3 * 2^-24 relative, the products within one more rounding each, and exactly where the
        # factor is 1
        for limit in (0.99, 0.05):
            mx = wav.abs().max()
            ref = wav * min(limit / mx, 1)
            got = wav * R.rescale_factor(wav, limit)
            assert bool(((got - ref).abs() <= 5 * R.U * ref.abs()).all()), (n, limit)
            if float(mx) <= limit:
                assert torch.equal(got, wav) and torch.equal(ref, wav)
            assert float(R.rescale_factor(wav, limit)) == float(min(torch.tensor(limit, dtype=torch.float32) / mx, 1))
        assert R.peak64(wav[0].numpy()) == float(wav.abs().max())
    assert float(R.rescale_factor(torch.zeros(5), 0.99)) == 1.0
    assert R.rms_bound(1) == 3 * 2.0 ** -24 and R.rms_bound(4097) == 16 * 2.0 ** -24
