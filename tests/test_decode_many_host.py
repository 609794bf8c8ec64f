"""The grouping policy of WavTokenizer.decode_many (mixed_length.group_frames) and the constants of the mixed-length decode
entry point, without a GPU."""
import os
import random
import re

from wavtokenizer_amd.mixed_length import (MAX_FRAMES, MAX_GROUP, MAX_SCORE_CELLS, bucket_length, group_clips, group_frames,
                                           score_cells)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_groups(frames, groups):
    seen = sorted(i for _L_pad, idx in groups for i in idx)
    assert seen == list(range(len(frames)))                      # every index exactly once
    for L_pad, idx in groups:
        assert 1 <= len(idx) <= MAX_GROUP
        assert max(frames[i] for i in idx) <= L_pad <= MAX_FRAMES
        assert len(idx) == 1 or score_cells(len(idx), L_pad) <= MAX_SCORE_CELLS


def test_score_cap_is_the_largest_measured_attention_workspace():
    assert MAX_SCORE_CELLS == 32 * 1200 * 1216 == score_cells(32, 1200)
    assert score_cells(1, 1) == 32 and score_cells(2, 33) == 2 * 33 * 64


def test_every_index_once_for_random_lengths():
    rng = random.Random(1)
    for n in (0, 1, 2, 20, 64, 65, 300):
        frames = [rng.randint(1, 1500) for _ in range(n)]
        groups = group_frames(frames)
        _check_groups(frames, groups)
        for L_pad, idx in groups:                                # sorted by length, at most half of a call is bucket padding
            assert [frames[i] for i in idx] == sorted(frames[i] for i in idx)
            assert bucket_length(frames[idx[-1]], 1) <= 2 * frames[idx[0]] or len(idx) == 1


def test_sixty_four_long_clips_are_split_by_the_score_cap():
    for L in (1200, 1281):
        frames = [L] * 64
        groups = group_frames(frames)
        _check_groups(frames, groups)
        L_pad = bucket_length(L, 1)                              # 1280 and 1408
        assert all(g[0] == L_pad for g in groups)
        fit = MAX_SCORE_CELLS // score_cells(1, L_pad)           # clips of this padded length under the cap
        assert 1 < fit < 64 and [len(idx) for _L, idx in groups] == [fit] * (64 // fit) + ([64 % fit] if 64 % fit else [])
    assert len(group_frames([100] * 64)) == 1                    # short clips: the 64-clip limit alone


def test_a_single_long_clip_forms_a_group_alone():
    groups = group_frames([12000])
    assert groups == [(12000, [0])] and score_cells(1, 12000) > MAX_SCORE_CELLS
    groups = group_frames([12000, 5, 12000, 6])
    _check_groups([12000, 5, 12000, 6], groups)
    assert sorted(len(idx) for _L, idx in groups) == [1, 1, 2]


def test_encode_grouping_is_unchanged_by_the_cap_parameter():
    rng = random.Random(3)
    lengths = [rng.randint(500, 200000) for _ in range(200)]
    assert group_clips(lengths, 600) == group_clips(lengths, 600, max_cells=0)
    groups, solo = group_clips(lengths, 600)
    assert sorted([i for _T, idx in groups for i in idx] + solo) == list(range(200))


def test_header_and_capi_constants_agree():
    from wavtokenizer_amd import _capi          # (binds the built library: the entry point must be exported)
    with open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")) as f:
        h = f.read()

    def const(name):
        return int(re.search(r"\b%s\s*=\s*(\d+)" % name, h).group(1))

    assert const("WT_PLAN_DECODE_MIXED") == _capi.WT_PLAN_DECODE_MIXED == 5
    assert const("WT_STATUS_BIT_LENGTH") == _capi.WT_STATUS_BIT_LENGTH == 4
    for name, val in (("TRANSPOSE_MIXED", 16), ("GN_MIXED", 17), ("DWCONV_LN_MIXED", 18), ("SOFTMAX_REG_MIXED", 19),
                      ("SOFTMAX_RMW_MIXED", 20), ("ISTFT_OLA_MIXED", 21)):
        assert const("WT_OPK_" + name) == val and _capi.WT_OPK_NAMES[val] == name.lower()
    assert "wt_decode_mixed" in _capi.EXPORTS and re.search(r"\bint wt_decode_mixed\(", h)
    assert _capi.lib.wt_decode_mixed.argtypes is not None and len(_capi.lib.wt_decode_mixed.argtypes) == 7
    # the lengths pointer is the last field of wt_op_desc on both sides
    assert _capi.WtOpDesc._fields_[-1][0] == "lengths"
    assert re.search(r"const int32_t\* lengths;[^}]*\}\s*wt_op_desc;", h)
