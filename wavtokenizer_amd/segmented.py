"""Long recordings in overlapping segments (the reference's EncodecModel.encode / .decode, encoder/model.py:122-191): the segment
geometry and the container WavTokenizer.encode_codes_segmented(_many) returns and decode_pcm_segmented(_many) takes.  Pure
functions of lengths and plain tensors (no GPU), so that every argument error is raised before any GPU work and the geometry is
tested on its own.

A recording of `length` samples at the codec rate is cut at offsets range(0, length, stride) into segments of at most
segment_length samples (model.py:142-143); every segment is encoded and decoded as a clip of its own and the decoded segments are
cross-faded by the reference's linear overlap-add (encoder/utils.py:17-56).  Near a cut the codes of a segmented recording
differ from the codes of the whole recording by construction: each segment starts from the encoder's padding and a fresh LSTM
state."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .mixed_length import MAX_FRAMES


def _int(v, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer")
    return int(v)


def segment_plan(length: int, segment_length: int, stride: int) -> Tuple[List[int], List[int]]:
    """(offsets, lengths) of the segments EncodecModel.encode cuts (model.py:142-143): offsets range(0, length, stride),
    lengths[i] = min(segment_length, length - offsets[i]).  With stride < segment_length several trailing segments can be short;
    all of them end at `length`.  ValueError for a length, segment length or stride below 1 and for stride > segment_length
    (samples between two segments would belong to none)."""
    length, segment_length, stride = _int(length, "length"), _int(segment_length, "segment_length"), _int(stride, "stride")
    if length < 1:
        raise ValueError("a recording needs at least one sample")
    if segment_length < 1 or stride < 1:
        raise ValueError("segment_length and stride must be positive")
    if stride > segment_length:
        raise ValueError("stride beyond segment_length leaves uncovered samples")
    offsets = list(range(0, length, stride))
    return offsets, [min(segment_length, length - o) for o in offsets]


def check_geometry(arch, length: int, segment_length: int, stride: int) -> Tuple[List[int], List[int], List[int]]:
    """segment_plan plus the frames of every segment under `arch`, (offsets, lengths, frames), after the checks that need the
    architecture: ValueError for an ISTFT with padding="center" (a decoded segment then has (L - 1) * hop samples, fewer than
    the segment it must cover) and for a segment beyond the MAX_FRAMES frames a plan takes."""
    offsets, lengths = segment_plan(length, segment_length, stride)
    if arch.padding != "same":
        raise ValueError('segmented coding needs an ISTFT head with padding="same": with "center" a decoded segment is shorter '
                         "than the segment it must cover")
    if arch.frames(lengths[0]) > MAX_FRAMES:
        raise ValueError(f"a segment of {lengths[0]} samples has more than {MAX_FRAMES} frames: choose a shorter segment_length")
    return offsets, lengths, [arch.frames(n) for n in lengths]


class SegmentedCodes:
    """The codes of one recording cut into segments.

        codes            flat integer tensor: the segments' codes back to back (one codebook)
        offsets          int64 [n_seg + 1] on the CPU: segment i is codes[offsets[i]:offsets[i + 1]]
        length           samples of the recording at the codec rate
        segment_length   samples of a full segment
        stride           samples between the starts of two segments
        scales           None, or fp32 (n_seg,): the divisor each segment was normalised by before it was encoded
                         (encode_codes_segmented(normalize=...), Encodec's (codes, scale) frames); decode_pcm_segmented multiplies
                         segment i's decoded samples by scales[i] before the cross-fade

    Built by WavTokenizer.encode_codes_segmented(_many), or by hand from a caller's own codes (a language model's output): the
    constructor takes the flat form, from_segments the list form.  validate(arch) is what decode_pcm_segmented checks."""
    __slots__ = ("codes", "offsets", "length", "segment_length", "stride", "scales")

    def __init__(self, codes: torch.Tensor, offsets, length: int, segment_length: int, stride: int, scales: Optional[torch.Tensor] = None):
        if not isinstance(codes, torch.Tensor) or codes.dim() != 1 or codes.is_floating_point() or codes.is_complex() or codes.dtype == torch.bool:
            raise ValueError("SegmentedCodes: codes must be a flat integer tensor")
        offsets = torch.as_tensor(offsets, dtype=torch.int64, device="cpu")
        if offsets.dim() != 1 or offsets.numel() < 2:
            raise ValueError("SegmentedCodes: offsets must be a 1-D tensor of n_seg + 1 entries")
        self.codes, self.offsets = codes, offsets
        self.length, self.segment_length, self.stride = _int(length, "length"), _int(segment_length, "segment_length"), _int(stride, "stride")
        if scales is not None and (not isinstance(scales, torch.Tensor) or scales.dim() != 1 or not scales.is_floating_point()):
            raise ValueError("SegmentedCodes: scales must be None or a 1-D floating-point tensor, one entry per segment")
        self.scales = scales

    @classmethod
    def from_segments(cls, segments: Sequence[torch.Tensor], length: int, segment_length: int, stride: int,
                      scales: Optional[torch.Tensor] = None) -> "SegmentedCodes":
        """The list form: segments[i] holds segment i's codes as (L_i,), (1, L_i) or (1, 1, L_i); they are copied into one flat
        tensor.  scales: None, or the segments' scales as one tensor (n_seg,) or a sequence of one-element tensors / numbers."""
        segments = list(segments)
        if not segments:
            raise ValueError("SegmentedCodes: no segments")
        flat = []
        for s in segments:
            if not isinstance(s, torch.Tensor) or s.dim() not in (1, 2, 3) or any(int(n) != 1 for n in s.shape[:-1]) or s.shape[-1] < 1:
                raise ValueError("SegmentedCodes: a segment is a tensor (L,), (1, L) or (1, 1, L) with L >= 1")
            flat.append(s.reshape(-1))
        offsets = [0]
        for s in flat:
            offsets.append(offsets[-1] + int(s.numel()))
        if scales is not None and not isinstance(scales, torch.Tensor):
            scales = list(scales)
            scales = (torch.cat([v.reshape(-1).to(torch.float32) for v in scales]) if scales and isinstance(scales[0], torch.Tensor)
                      else torch.tensor(scales, dtype=torch.float32))
        return cls(torch.cat(flat), offsets, length, segment_length, stride, scales)

    @property
    def n_segments(self) -> int:
        return int(self.offsets.numel()) - 1

    def segments(self) -> List[torch.Tensor]:
        """The segments' codes as (1, 1, L_i) views of the flat tensor, L_i = arch.frames(lengths[i])."""
        o = self.offsets.tolist()
        return [self.codes[o[i]:o[i + 1]].view(1, 1, -1) for i in range(len(o) - 1)]

    def validate(self, arch) -> Tuple[List[int], List[int], List[int]]:
        """check_geometry(arch, length, segment_length, stride), after checking that offsets are the prefix sums of its frames and
        that codes holds exactly that many and scales, when given, one entry per segment: ValueError otherwise."""
        offsets, lengths, frames = check_geometry(arch, self.length, self.segment_length, self.stride)
        want = [0]
        for L in frames:
            want.append(want[-1] + L)
        if self.offsets.tolist() != want:
            raise ValueError("SegmentedCodes: offsets contradict segment_plan(length, segment_length, stride) under this architecture")
        if int(self.codes.numel()) != want[-1]:
            raise ValueError("SegmentedCodes: codes does not hold offsets[-1] entries")
        if self.scales is not None and int(self.scales.numel()) != len(frames):
            raise ValueError("SegmentedCodes: scales does not hold one entry per segment")
        return offsets, lengths, frames

    def __repr__(self) -> str:
        return (f"SegmentedCodes(n_segments={self.n_segments}, length={self.length}, segment_length={self.segment_length}, "
                f"stride={self.stride}, codes={tuple(self.codes.shape)} on {self.codes.device}"
                + ("" if self.scales is None else f", scales={tuple(self.scales.shape)} on {self.scales.device}") + ")")
