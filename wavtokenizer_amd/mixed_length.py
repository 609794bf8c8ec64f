"""Grouping policy of WavTokenizer.encode_infer_many, decode_many and decode_codes_many: which clips share a mixed-length call, and how long its
padded staging tensor is.  Pure functions of the clip lengths (no GPU), so the policy is tested on its own.

A mixed-length call returns for every clip the bits a call of its own length returns (the kernels read each clip's length on
the device), so grouping and bucketing change only the cost: a bucket is a coarse padded length that many calls share, which
lets them reuse one plan (and, for small groups, one recorded graph) instead of building one per length."""
from __future__ import annotations

from typing import List, Sequence, Tuple

MAX_FRAMES = 12000       # frames per clip of one plan (wt_plan_create): a bucket never goes past it
MIN_CLIP = 1024          # the shortest clip a mixed-length plan takes (wt_plan_min_clip_length: the fused stage-1 kernel)
MAX_GROUP = 64           # clips per call: the wt_ingest / wt_emit descriptor blocks and the plan buckets are sized for it (the
                         # persistent LSTM gives every clip the bits of a call of its own at any size it takes, up to 128)
BUCKET_STEPS = 8         # buckets per octave of length: at most 1/8 of a call is padding from the bucket


def bucket_length(T: int, hop: int) -> int:
    """T rounded up to a multiple of hop * 2^e, with e chosen so that there are BUCKET_STEPS such multiples per octave
    (at least one hop): 3 s at hop 320 (48 000 samples) -> 51 200 (ten multiples of 5 120)."""
    if T < 1 or hop < 1:
        raise ValueError("length and hop must be positive")
    q = hop
    while (T + q - 1) // q > 2 * BUCKET_STEPS - 1:
        q *= 2
    return -(-T // q) * q


MAX_SCORE_CELLS = 32 * 1200 * 1216   # attention score cells (B * L_pad * Lp, held twice as floats) per decode call: the largest
                                     # attention workspace this project measures (the 32 x 30 s row of bench.py --full)


def score_cells(B: int, L_pad: int) -> int:
    """Cells of the decoder's attention score matrix for B clips of L_pad frames (row pitch: L_pad rounded up to 32)."""
    return B * L_pad * (-(-L_pad // 32) * 32)


def group_clips(lengths: Sequence[int], hop: int, min_clip: int = MIN_CLIP, max_group: int = MAX_GROUP, max_cells: int = 0
                ) -> Tuple[List[Tuple[int, List[int]]], List[int]]:
    """(groups, solo): groups = [(padded length, clip indices)], solo = indices of the clips shorter than min_clip (they run
    one at a time through encode_infer).  Clips are taken in order of length (ties in input order); a group closes at
    max_group clips or when the next clip's bucket is more than twice the group's first clip (more than half of the call
    would be padding).  max_cells > 0 (decode, lengths in frames): a group also closes before the clip with which its score
    matrix (score_cells at the padded length) would exceed max_cells; a single clip always forms a group.  Every clip index
    appears exactly once."""
    def padded(T: int) -> int:
        return max(T, min(bucket_length(T, hop), MAX_FRAMES * hop))

    def over_cells(n: int, T: int) -> bool:
        return max_cells > 0 and score_cells(n, padded(T)) > max_cells

    order = sorted(range(len(lengths)), key=lambda i: (int(lengths[i]), i))
    solo = [i for i in order if int(lengths[i]) < min_clip]
    groups: List[Tuple[int, List[int]]] = []
    cur: List[int] = []
    for i in order:
        T = int(lengths[i])
        if T < min_clip:
            continue
        if cur and (len(cur) >= max_group or bucket_length(T, hop) > 2 * int(lengths[cur[0]]) or over_cells(len(cur) + 1, T)):
            groups.append((padded(int(lengths[cur[-1]])), cur))
            cur = []
        cur.append(i)
    if cur:
        groups.append((padded(int(lengths[cur[-1]])), cur))
    return groups, solo


def group_frames(frames: Sequence[int], max_group: int = MAX_GROUP) -> List[Tuple[int, List[int]]]:
    """Grouping of WavTokenizer.decode_many and decode_codes_many: group_clips in units of frames (hop 1, every clip of one frame or more is taken)
    with the score-cell cap.  Returns [(padded frames, clip indices)]; every index appears exactly once."""
    groups, solo = group_clips(frames, 1, min_clip=1, max_group=max_group, max_cells=MAX_SCORE_CELLS)
    assert not solo
    return groups
