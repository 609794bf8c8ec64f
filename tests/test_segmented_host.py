"""The host side of long recordings in segments without a GPU: the segment geometry (wavtokenizer_amd/segmented.py) against plain
slicing, the SegmentedCodes container, every argument error of encode_codes_segmented(_many) and decode_pcm_segmented(_many) on a
model that was never loaded, the new exports on both sides of the C ABI and wt_overlap_add_ragged's refusals (made before any
device call, with pointers that are not even valid)."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ geometry
def test_segment_plan_is_the_slicing_of_the_reference_loop():
    from wavtokenizer_amd.segmented import segment_plan
    n = 0
    for S in range(1, 13):
        for stride in range(1, S + 1):
            for length in range(1, 41):
                x = np.arange(length)
                want = [x[off:off + S] for off in range(0, length, stride)]          # encoder/model.py:142-143
                offsets, lengths = segment_plan(length, S, stride)
                assert offsets == [int(w[0]) for w in want] and lengths == [len(w) for w in want], (S, stride, length)
                assert all(o + n_ <= length for o, n_ in zip(offsets, lengths))
                assert all(o + n_ == length for o, n_ in zip(offsets, lengths) if n_ < S)      # short segments end at `length`
                covered = np.zeros(length, bool)
                for o, n_ in zip(offsets, lengths):
                    covered[o:o + n_] = True
                assert covered.all()
                n += 1
    assert n == 78 * 40
    assert segment_plan(np.int64(10), np.int32(4), 3) == ([0, 3, 6, 9], [4, 4, 4, 1])


def test_frames_per_segment_follow_the_architecture():
    from wavtokenizer_amd import NAMED_ARCHS
    from wavtokenizer_amd.segmented import check_geometry, segment_plan
    for name, hop in (("hop600", 600), ("hop320", 320)):
        arch = NAMED_ARCHS[name]
        for length, S, stride in ((3601, 4800, 3600), (12000, 4800, 1500), (253200, 4800, 3600), (48000, 17777, 11111), (500, 4800, 3600)):
            offsets, lengths, frames = check_geometry(arch, length, S, stride)
            assert (offsets, lengths) == segment_plan(length, S, stride)
            assert frames == [arch.frames(n) for n in lengths] == [-(-n // hop) for n in lengths]
    assert check_geometry(NAMED_ARCHS["hop600"], 3601, 4800, 3600)[2] == [7, 1]


def test_geometry_refusals():
    from wavtokenizer_amd import ARCH_HOP320, ARCH_HOP600
    from wavtokenizer_amd.mixed_length import MAX_FRAMES
    from wavtokenizer_amd.segmented import check_geometry, segment_plan
    for length, S, stride in ((10, 0, 1), (10, 4, 0), (10, -4, 2), (10, 4, -1), (10, 4, 5), (0, 4, 2), (-3, 4, 2),
                              (10.0, 4, 2), (10, 4.0, 2), (10, 4, True)):
        with pytest.raises(ValueError):
            segment_plan(length, S, stride)
    # a segment beyond MAX_FRAMES frames: 12 000 frames are 7 200 000 samples at hop 600 and 3 840 000 at hop 320
    assert check_geometry(ARCH_HOP600, 8_000_000, MAX_FRAMES * 600, 600)[2][0] == MAX_FRAMES
    with pytest.raises(ValueError, match="frames"):
        check_geometry(ARCH_HOP600, 8_000_000, MAX_FRAMES * 600 + 1, 600)
    with pytest.raises(ValueError, match="frames"):
        check_geometry(ARCH_HOP320, 8_000_000, MAX_FRAMES * 320 + 1, 320)
    assert len(check_geometry(ARCH_HOP600, 1000, MAX_FRAMES * 600 + 1, 600)[0]) == 2      # (no such segment exists in a short recording)
    with pytest.raises(ValueError, match="center"):
        check_geometry(dataclasses.replace(ARCH_HOP600, padding="center"), 10000, 4800, 3600)


# ------------------------------------------------------------------------------------------------ the container
def test_segmented_codes_round_trip_between_list_and_flat_form():
    from wavtokenizer_amd import ARCH_HOP600
    from wavtokenizer_amd.segmented import SegmentedCodes, check_geometry
    length, S, stride = 12000, 4800, 1500
    _offs, _lens, frames = check_geometry(ARCH_HOP600, length, S, stride)
    assert frames == [8, 8, 8, 8, 8, 8, 5, 3]
    rng = np.random.default_rng(0)
    flat = torch.from_numpy(rng.integers(0, 4096, size=sum(frames)))
    bounds = np.concatenate([[0], np.cumsum(frames)])
    sc = SegmentedCodes(flat, bounds, length, S, stride)
    assert sc.n_segments == 8 and sc.offsets.dtype == torch.int64 and sc.offsets.device.type == "cpu"
    parts = sc.segments()
    assert [tuple(p.shape) for p in parts] == [(1, 1, L) for L in frames]
    assert all(p.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for p in parts)      # views
    assert sc.validate(ARCH_HOP600)[2] == frames
    for form in (lambda p: p, lambda p: p[0], lambda p: p[0, 0]):                           # (1, 1, L), (1, L) and (L,)
        back = SegmentedCodes.from_segments([form(p) for p in parts], length, S, stride)
        assert torch.equal(back.codes, flat) and torch.equal(back.offsets, sc.offsets)
        assert (back.length, back.segment_length, back.stride) == (length, S, stride)
        back.validate(ARCH_HOP600)
    # by hand, from a caller's own codes in another integer type
    own = SegmentedCodes(flat.to(torch.int32), bounds.tolist(), length, S, stride)
    own.validate(ARCH_HOP600)
    assert "n_segments=8" in repr(own)


def _good(length=12000, S=4800, stride=1500):
    from wavtokenizer_amd import ARCH_HOP600
    from wavtokenizer_amd.segmented import SegmentedCodes, check_geometry
    frames = check_geometry(ARCH_HOP600, length, S, stride)[2]
    return SegmentedCodes(torch.zeros(sum(frames), dtype=torch.int64), [0] + np.cumsum(frames).tolist(), length, S, stride), frames


def test_segmented_codes_refuses_what_contradicts_the_plan():
    from wavtokenizer_amd import ARCH_HOP320, ARCH_HOP600
    from wavtokenizer_amd.segmented import SegmentedCodes
    sc, frames = _good()
    bounds = [0] + np.cumsum(frames).tolist()
    n = sum(frames)
    z = torch.zeros(n, dtype=torch.int64)
    for bad in (lambda: SegmentedCodes(z.float(), bounds, 12000, 4800, 1500),               # floating-point codes
                lambda: SegmentedCodes(z.bool(), bounds, 12000, 4800, 1500),
                lambda: SegmentedCodes(z.view(1, -1), bounds, 12000, 4800, 1500),           # not flat
                lambda: SegmentedCodes([1, 2, 3], bounds, 12000, 4800, 1500),               # not a tensor
                lambda: SegmentedCodes(z, [0], 12000, 4800, 1500),                          # no segment
                lambda: SegmentedCodes(z, [bounds], 12000, 4800, 1500),
                lambda: SegmentedCodes(z, bounds, 12000.0, 4800, 1500),
                lambda: SegmentedCodes.from_segments([], 12000, 4800, 1500),
                lambda: SegmentedCodes.from_segments([torch.zeros((2, 8), dtype=torch.int64)], 12000, 4800, 1500),
                lambda: SegmentedCodes.from_segments([torch.zeros((1, 0), dtype=torch.int64)], 12000, 4800, 1500)):
        with pytest.raises(ValueError):
            bad()
    for kw in (dict(length=12001), dict(length=11400), dict(length=10500), dict(stride=1400), dict(stride=3000),
               dict(segment_length=4200), dict(segment_length=1499), dict(stride=0), dict(length=0)):
        args = dict(length=12000, segment_length=4800, stride=1500)
        args.update(kw)
        with pytest.raises(ValueError):
            SegmentedCodes(z, bounds, **args).validate(ARCH_HOP600)
    with pytest.raises(ValueError, match="contradict"):
        sc.validate(ARCH_HOP320)                                                            # (other frames per segment)
    moved = list(bounds)
    moved[3] += 1
    with pytest.raises(ValueError, match="contradict"):
        SegmentedCodes(z, moved, 12000, 4800, 1500).validate(ARCH_HOP600)
    with pytest.raises(ValueError, match="contradict"):
        SegmentedCodes(z, bounds[:-1], 12000, 4800, 1500).validate(ARCH_HOP600)
    with pytest.raises(ValueError, match="offsets\\[-1\\]"):
        SegmentedCodes(torch.zeros(n + 1, dtype=torch.int64), bounds, 12000, 4800, 1500).validate(ARCH_HOP600)


# ------------------------------------------------------------------------------------------------ the methods' argument errors
def _unloaded(arch=None):
    """A model on the CPU whose engine must never be asked for: any GPU work would start there."""
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(arch or ARCH_HOP600)

    def no_gpu():
        raise AssertionError("GPU work was started")
    m._ensure_engine = no_gpu
    return m


def test_encode_codes_segmented_validates_before_any_gpu_work():
    from wavtokenizer_amd import ARCH_HOP600
    m = _unloaded()
    wav = torch.zeros(30000)
    long_ = torch.zeros(2_500_000, dtype=torch.int16)        # 7 500 000 samples once resampled from 8 kHz: the cut comes second
    for clips, S, stride, kw in (([wav], 0, 1, {}), ([wav], 4800, 0, {}), ([wav], 4800, 4801, {}), ([wav], -1, -1, {}),
                                 ([wav], 4800.0, 3600, {}), ([], 4800, 4801, {}),
                                 ([long_], 12000 * 600 + 1, 12000 * 600 + 1, dict(sample_rates=8000)),      # a segment beyond MAX_FRAMES
                                 ([wav.double()], 4800, 3600, {}), ([wav.view(1, 1, -1)], 4800, 3600, {}),
                                 ([torch.zeros((3, 100))], 4800, 3600, {}), ([torch.zeros(0)], 4800, 3600, {}),
                                 ([wav, wav], 4800, 3600, dict(sample_rates=[24000])),
                                 ([wav], 4800, 3600, dict(sample_rates=0)),
                                 ([[0.0] * 10], 4800, 3600, {})):
        with pytest.raises(ValueError):
            m.encode_codes_segmented_many(clips, S, stride, **kw)
    with pytest.raises(ValueError):
        m.encode_codes_segmented(wav, 4800, 4801)
    with pytest.raises(ValueError):
        m.encode_codes_segmented(wav, 4800, 3600, sample_rate=-5)
    center = _unloaded(dataclasses.replace(ARCH_HOP600, padding="center"))
    with pytest.raises(ValueError, match="center"):
        center.encode_codes_segmented_many([wav], 4800, 3600)
    with pytest.raises(ValueError, match="center"):
        center.encode_codes_segmented(wav, 4800, 3600)
    assert m.encode_codes_segmented_many([], 4800, 3600) == []
    with pytest.raises(AssertionError, match="GPU work"):                                   # (a good call does get that far)
        m.encode_codes_segmented_many([wav], 4800, 3600)


def test_decode_pcm_segmented_validates_before_any_gpu_work():
    from wavtokenizer_amd import ARCH_HOP600
    from wavtokenizer_amd.segmented import SegmentedCodes
    m = _unloaded()
    sc, frames = _good()
    bounds = sc.offsets.tolist()
    wrong = SegmentedCodes(sc.codes, bounds, 12001, 4800, 1500)
    uncovered = SegmentedCodes(torch.zeros(4, dtype=torch.int64), [0, 2, 4], 2400, 1200, 1201)
    for segs, kw in (([wrong], {}), ([sc, wrong], {}), ([uncovered], {}), ([sc.codes], {}), ([sc.segments()], {}),
                     ([sc], dict(dtype=torch.float64)), ([sc], dict(dtype=torch.int32)),
                     ([sc], dict(channels=0)), ([sc], dict(channels=3)), ([sc], dict(channels=True)), ([sc, sc], dict(channels=[1])),
                     ([sc], dict(limit=0.0)), ([sc], dict(limit=1.5)), ([sc], dict(limit=float("nan"))),
                     ([sc, sc], dict(sample_rates=[24000])), ([sc], dict(sample_rates=0)), ([sc], dict(sample_rates=7999)),
                     ([sc], dict(device="meta"))):
        with pytest.raises(ValueError):
            m.decode_pcm_segmented_many(segs, bandwidth_id=0, **kw)
    with pytest.raises(ValueError):
        m.decode_pcm_segmented(wrong, bandwidth_id=0)
    with pytest.raises(ValueError):
        m.decode_pcm_segmented(sc, channels=[1], bandwidth_id=0)
    with pytest.raises(ValueError):
        m.decode_pcm_segmented(sc, sample_rate=7999, bandwidth_id=0)
    center = _unloaded(dataclasses.replace(ARCH_HOP600, padding="center"))
    with pytest.raises(ValueError, match="center"):
        center.decode_pcm_segmented_many([sc], bandwidth_id=0)
    assert m.decode_pcm_segmented_many([], bandwidth_id=0) == []
    flat, offs = m.decode_pcm_segmented_many([], packed=True, dtype=torch.float32, bandwidth_id=0)
    assert flat.numel() == 0 and flat.dtype == torch.float32 and offs.tolist() == [0]
    with pytest.raises(AssertionError, match="GPU work"):
        m.decode_pcm_segmented_many([sc], bandwidth_id=0)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_and_capi_agree_on_the_new_exports():
    from wavtokenizer_amd import _capi          # (binds the built library: the entry points must be exported)
    with open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")) as f:
        h = f.read()
    for name, ret, nargs in (("wt_overlap_add_ragged", "int", 4), ("wt_overlap_add_ragged_workspace_bytes", "size_t", 1)):
        assert name in _capi.EXPORTS
        decl = re.search(r"\b%s\s+%s\(([^;]*?)\);" % (ret, name), h, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        fn = getattr(_capi.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    body = re.search(r"typedef struct \{([^}]*)\} wt_overlap_add_clip;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            fields += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
    assert fields == [f[0] for f in _capi.WtOverlapAddClip._fields_], fields
    assert fields == ["rows", "n_frames", "frame_len", "stride", "total", "weight", "out"]
    assert ctypes.sizeof(_capi.WtOverlapAddClip) == 56
    ws = _capi.lib.wt_overlap_add_ragged_workspace_bytes
    assert ws(0) == 0 and ws(-3) == 0
    assert 0 < ws(1) < ws(2) < ws(64) and ws(64) == 64 * ws(1) and ws(1) % 8 == 0


def test_overlap_add_ragged_refuses_bad_descriptors_before_any_hip_call():
    from wavtokenizer_amd import _capi
    fake = 1 << 20                                           # not a valid address: nothing may be dereferenced
    good = dict(rows=fake, n_frames=3, frame_len=1200, stride=900, total=2500, weight=fake * 2, out=fake * 3)

    def rc(second=None, ws=fake * 4, B=2, **kw):
        clips = (_capi.WtOverlapAddClip * 2)()
        for c in clips:
            for k, v in good.items():
                setattr(c, k, v)
        for k, v in kw.items():
            setattr(clips[0], k, v)
        for k, v in (second or {}).items():
            setattr(clips[1], k, v)
        return _capi.lib.wt_overlap_add_ragged(clips, B, ws, None), _capi.lib.wt_last_error().decode()

    cases = [(dict(rows=None), "null row table"), (dict(weight=None), "null weight"), (dict(out=None), "null destination"),
             (dict(n_frames=0), "n_frames < 1"), (dict(n_frames=-2), "n_frames < 1"),
             (dict(total=0), "total < 1"), (dict(total=-5), "total < 1"),
             (dict(frame_len=0), "frame_len < 1"), (dict(frame_len=-1), "frame_len < 1"),
             (dict(stride=0), "stride < 1"), (dict(stride=-900), "stride < 1"),
             (dict(n_frames=2), "ceil(total / stride)"), (dict(n_frames=4), "ceil(total / stride)"),
             (dict(total=2701), "ceil(total / stride)"),                                    # (a fourth frame would begin)
             (dict(stride=1201, total=3000), "uncovered"),                                  # three frames of 1200 every 1201
             (dict(frame_len=600), "uncovered"),
             (dict(stride=1000, n_frames=2, total=1999, frame_len=1000), None),              # (good: see below)
             (dict(stride=500, n_frames=5, total=2500, frame_len=499), "uncovered"),
             (dict(stride=900, n_frames=1, total=900, frame_len=899), "beyond the last frame"),
             (dict(stride=5000, n_frames=1, total=1201), "beyond the last frame"),          # one frame, longer than frame_len
             (dict(rows=fake + 4), "misaligned"), (dict(weight=fake * 2 + 2), "misaligned"), (dict(out=fake * 3 + 1), "misaligned")]
    other = dict(n_frames=0)
    for kw, msg in cases:
        if msg is None:
            continue
        for second in (None, kw):                            # as the first recording of the call and behind a good one
            code, err = rc(second=second, **({} if second else kw))
            assert code == _capi.WT_ERR_INVALID and msg in err, (kw, err)
            if second:
                assert "recording 1" in err
    code, err = rc(ws=None)
    assert code == _capi.WT_ERR_INVALID and "bad argument" in err
    code, err = rc(ws=fake * 4 + 4)
    assert code == _capi.WT_ERR_INVALID and "misaligned" in err
    assert _capi.lib.wt_overlap_add_ragged(None, 2, fake, None) == _capi.WT_ERR_INVALID
    clips = (_capi.WtOverlapAddClip * 1)()
    assert _capi.lib.wt_overlap_add_ragged(clips, 0, fake, None) == _capi.WT_ERR_INVALID
    assert _capi.lib.wt_overlap_add_ragged(clips, 65536, fake, None) == _capi.WT_ERR_INVALID
    # what is NOT refused, shown by the refusal that comes next in the order of the checks (recording 1's): stride = frame_len,
    # a single frame shorter than its stride, a last frame of one sample, eight frames deep
    for kw in (dict(stride=1000, n_frames=2, total=1999, frame_len=1000), dict(stride=5000, n_frames=1, total=1200),
               dict(stride=3600, n_frames=2, total=3601, frame_len=4800), dict(stride=1, n_frames=12, total=12, frame_len=8)):
        code, err = rc(second=other, **kw)
        assert code == _capi.WT_ERR_INVALID and "recording 1: n_frames < 1" in err, (kw, err)
