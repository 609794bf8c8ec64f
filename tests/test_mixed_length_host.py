"""Mixed-length encode, host side (no GPU): the SConv1d geometry the plans and the device geometry step share, against the
reference's padding rules, and the grouping / bucketing policy of encode_infer_many."""
import ctypes
import math
import random

import pytest

from wavtokenizer_amd.config import NAMED_ARCHS
from wavtokenizer_amd.mixed_length import MAX_FRAMES, MAX_GROUP, MIN_CLIP, bucket_length, group_clips


def _reference_geometry(T, k, stride, dil):
    """encoder/modules/conv.py: SConv1d.forward (non-causal), get_extra_padding_for_conv1d and pad1d's reflect rule."""
    keff = (k - 1) * dil + 1
    padding_total = keff - stride
    n_frames = (T - keff + padding_total) / stride + 1
    ideal_length = (math.ceil(n_frames) - 1) * stride + (keff - padding_total)
    extra = ideal_length - T
    padding_right = padding_total // 2
    padding_left = padding_total - padding_right
    max_pad = max(padding_left, padding_right + extra)
    Tp = T + (max_pad - T + 1 if T <= max_pad else 0)
    t_out = (T + padding_left + padding_right + extra - keff) // stride + 1
    return padding_left, padding_right + extra, t_out, Tp


def _geometry(T, k, stride, dil):
    from wavtokenizer_amd import _capi
    out = (ctypes.c_int32 * 4)()
    _capi.check(_capi.lib.wt_sconv_geometry(T, k, stride, dil, out), "wt_sconv_geometry")
    return tuple(out)


def test_shared_geometry_matches_the_reference_padding_rules():
    Ts = list(range(1, 130)) + [511, 1023, 1024, 1025, 4799, 4800, 4801, 72000, 720000, 3840000]
    n = 0
    for k, stride, dil in [(1, 1, 1), (3, 1, 1), (3, 1, 2), (3, 1, 3), (7, 1, 1), (4, 2, 1), (8, 4, 1), (10, 5, 1),
                           (12, 6, 1), (16, 8, 1), (5, 2, 2), (9, 3, 1)]:
        for T in Ts:
            assert _geometry(T, k, stride, dil) == _reference_geometry(T, k, stride, dil), (T, k, stride, dil)
            n += 1
    assert n > 1500


@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_geometry_chain_gives_the_frame_count(name):
    """The encoder's down convs (k = 2r, stride r) and final k7 conv, chained as the mixed-length geometry step chains them,
    end at arch.frames(T) frames."""
    arch = NAMED_ARCHS[name]
    for T in list(range(1024, 1300)) + [4799, 4800, 4801, 72000, 720001]:
        Tc = T
        for r in arch.enc_ratios:
            assert _geometry(Tc, 3, 1, 1)[2] == Tc and _geometry(Tc, 1, 1, 1)[2] == Tc
            Tc = _geometry(Tc, 2 * r, r, 1)[2]
        assert _geometry(Tc, 7, 1, 1)[2] == Tc == arch.frames(T), (T, Tc)


def test_geometry_refuses_bad_arguments():
    from wavtokenizer_amd import _capi
    out = (ctypes.c_int32 * 4)()
    for args in [(0, 3, 1, 1), (10, 0, 1, 1), (10, 3, 0, 1), (10, 3, 1, 0), (10, 2, 4, 1)]:
        assert _capi.lib.wt_sconv_geometry(*args, out) == _capi.WT_ERR_INVALID, args


def test_mixed_plan_flag_and_entry_points_are_declared():
    from wavtokenizer_amd import _capi
    header = open(_capi.__file__.replace("wavtokenizer_amd/_capi.py", "include/wavtokenizer_amd.h")).read()
    assert "WT_PLAN_FLAG_MIXED_LENGTH = %d" % _capi.WT_PLAN_FLAG_MIXED_LENGTH in header
    for sym in ("wt_encode_mixed", "wt_plan_min_clip_length", "wt_sconv_geometry"):
        assert sym in _capi.EXPORTS and getattr(_capi.lib, sym) is not None
    assert _capi.lib.wt_plan_min_clip_length(None) == 0


@pytest.mark.parametrize("hop", [600, 320])
def test_buckets_are_coarse_and_cover_the_length(hop):
    prev = 0
    for T in list(range(1, 5000, 7)) + [72000, 480000, 720000, 3000000]:
        b = bucket_length(T, hop)
        assert b >= T and b % hop == 0 and b >= prev
        prev = b
        if T >= 8 * hop:
            assert (b - T) * 8 <= b, (T, b)                 # at most 1/8 of the padded length is padding
    distinct = {bucket_length(T, hop) for T in range(24000, 48000)}
    assert len(distinct) <= 9                               # one octave of lengths: a handful of plans


def test_grouping_policy():
    rng = random.Random(11)
    hop = 320
    lengths = [rng.randint(200, 20 * 24000) for _ in range(400)] + [MIN_CLIP, MIN_CLIP - 1, 5000, 5000]
    groups, solo = group_clips(lengths, hop)
    seen = sorted(solo + [i for _t, idx in groups for i in idx])
    assert seen == list(range(len(lengths)))                # every clip exactly once
    assert sorted(solo) == sorted(i for i, T in enumerate(lengths) if T < MIN_CLIP)
    last = 0
    for T_pad, idx in groups:
        assert 1 <= len(idx) <= MAX_GROUP
        ls = [lengths[i] for i in idx]
        assert ls == sorted(ls) and ls[0] >= last            # sorted by length, groups in order
        last = ls[-1]
        assert T_pad == bucket_length(max(ls), hop) and T_pad >= max(ls)
        assert T_pad <= 2 * ls[0]                            # at most half of a call is padding
    # ties keep input order; a long clip near the plan limit is not bucketed past it
    g, s = group_clips([5000, 3000, 5000], hop)
    assert s == [] and g == [(bucket_length(5000, hop), [1, 0, 2])]
    near = MAX_FRAMES * hop - 5
    g, _ = group_clips([near], hop)
    assert g == [(MAX_FRAMES * hop, [0])]
    g, _ = group_clips([2000] * 300, hop)
    assert [len(i) for _t, i in g] == [64, 64, 64, 64, 44]
    assert group_clips([], hop) == ([], [])
