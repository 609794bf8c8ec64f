"""Audio helpers on either side of the hot path, on the GPU (mirrors of the reference's encoder/utils.py).

    convert_audio(wav, sr, target_sr, target_channels)   encoder/utils.py:79-92   (mono target; resample on the GPU)
    to_pcm16(wav, rescale=False)                         encoder/utils.py:95-103 + the PCM_S 16 conversion of torchaudio.save
    linear_overlap_add(frames, stride)                   encoder/utils.py:17-56   (bit-identical)
    segment_offsets(length, segment_length, stride)      encoder/model.py:133-145 (the frame offsets of EncodecModel.encode)
    level(wav), level_many(wavs)                         peak and rms per clip (wt_level)
    normalize(wav, mode="peak" | "rms", target_db=0.0)   extract_features.py:27-28 / encoder/model.py:153-156 (wt_normalize_rows)
    loudness(wav, sample_rate), loudness_many(wavs, ...) integrated loudness in LUFS, ITU-R BS.1770-4 / EBU R 128 (wt_loudness)
    normalize(wav, mode="lufs", target_lufs=-23.0)       to a loudness target (wt_normalize_rows_lufs); with max_true_peak_db under a
                                                         true-peak ceiling (wt_normalize_rows_lufs_tp)
    true_peak(wav, sample_rate), true_peak_many(...)     true peak in dBTP and sample peak in dBFS, BS.1770-4 Annex 2 (wt_true_peak)
    loudness_range(wav, sample_rate), ..._many(...)      integrated, short-term and momentary loudness and the loudness range,
                                                         EBU Tech 3341 / 3342 (wt_loudness_range)
    r128_many(wavs, sample_rate)                         the summary of an R 128 meter per clip

All take and return torch tensors on the GPU; there is no CPU fallback.  Recordings of any length, from and to PCM, with codes in
between: WavTokenizer.encode_codes_segmented(_many) / decode_pcm_segmented(_many) (wavtokenizer_amd/segmented.py)."""
import ctypes
import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from ._capi import _need_gpu, _ptr, _stream, check, lib

_resamplers: Dict[Tuple[int, int, int], ctypes.c_void_p] = {}


_GPU_ONLY = "wavtokenizer_amd.audio runs on the GPU only (move the tensor with .to('cuda'))"


@functools.lru_cache(maxsize=None)
def resampler_geometry(sr: int, target_sr: int) -> Tuple[int, int, int, int]:
    """(orig, new, width, K) of the rate pair as wt_resampler_create derives them, on the host: the gcd-reduced rates, the half
    width and the taps per phase.  Raises ValueError for a pair the library refuses (a rate below 1, a ratio beyond the LDS
    window of the kernels), so that a caller can refuse its arguments before any GPU work.  The host twin of the rule in
    csrc/audio.hip (wt_resampler_create: width, K, the 15 000-float limit; wt_ingest: the 64 KiB of dynamic LDS): change them
    together (tests/test_encode_codes_host.py compares the two through wt_resampler_out_length and pinned pairs)."""
    import math
    sr, target_sr = int(sr), int(target_sr)
    if sr < 1 or target_sr < 1:
        raise ValueError("sample rates must be positive")
    g = math.gcd(sr, target_sr)
    orig, new = sr // g, target_sr // g
    if orig == new:
        return orig, new, 0, 1
    width = int(math.ceil(6 * orig / (min(orig, new) * 0.99)))
    K = 2 * width + orig
    if 256.0 * orig / new + K > 15000 or ((256 // new + 2) * orig + K) * 4 > 64 * 1024:
        raise ValueError(f"resampling {sr} -> {target_sr}: rate ratio too large for the LDS window")
    return orig, new, width, K


def resampled_length(sr: int, target_sr: int, length: int) -> int:
    """wt_resampler_out_length on the host: ceil(new * length / orig)."""
    orig, new, _w, _k = resampler_geometry(sr, target_sr)
    return -(-new * int(length) // orig)


def resampler(sr: int, target_sr: int, device_index: int) -> ctypes.c_void_p:
    """The wt_resampler of a rate pair on a device, created once per process."""
    key = (int(sr), int(target_sr), int(device_index))
    if key not in _resamplers:
        r = ctypes.c_void_p()
        check(lib.wt_resampler_create(int(sr), int(target_sr), int(device_index), ctypes.byref(r)), "wt_resampler_create")
        _resamplers[key] = r
    return _resamplers[key]


def convert_audio(wav: torch.Tensor, sr: int, target_sr: int, target_channels: int = 1) -> torch.Tensor:
    assert wav.dim() >= 2, "Audio tensor must have at least 2 dimensions"
    assert wav.shape[-2] in [1, 2], "Audio must be mono or stereo."
    if target_channels != 1:
        raise RuntimeError("only target_channels = 1 is implemented (what every caller of the codec path asks for)")
    _need_gpu(wav, _GPU_ONLY)
    *shape, channels, length = wav.shape
    dev = wav.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    r = resampler(sr, target_sr, idx)
    B = 1
    for s in shape:
        B *= int(s)
    x = wav.to(torch.float32).contiguous().view(max(B, 1), channels, length)
    Tout = int(lib.wt_resampler_out_length(r, length))
    out = torch.empty((max(B, 1), Tout), dtype=torch.float32, device=dev)
    check(lib.wt_convert_audio(r, _ptr(x), max(B, 1), channels, length, _ptr(out), _stream(dev)), "wt_convert_audio")
    return out.view(*shape, 1, Tout)


def to_pcm16(wav: torch.Tensor, rescale: bool = False, limit: float = 0.99) -> torch.Tensor:
    _need_gpu(wav, _GPU_ONLY)
    x = wav.to(torch.float32).contiguous()
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    ws = torch.zeros(1, dtype=torch.int32, device=x.device)
    check(lib.wt_pcm16(_ptr(x), x.numel(), float(limit), 1 if rescale else 0, _ptr(out), _ptr(ws), _stream(x.device)), "wt_pcm16")
    return out


def level_many(wavs: Sequence[torch.Tensor]) -> torch.Tensor:
    """Peak and rms of every clip: wavs is a sequence of non-empty 1-D fp32 tensors on one GPU; returns (n, 2) fp32 there, row i
    = (max |x|, sqrt(mean x^2)) of clip i.  One wt_level call (two launches) over all clips; the peak is exact, and a clip's rms
    has the same bits alone and in any batch (the order of its sum depends on its length alone)."""
    wavs = list(wavs)
    if not wavs:
        raise ValueError("level_many takes at least one clip")
    for w in wavs:
        if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] < 1 or w.dtype != torch.float32:
            raise ValueError("level_many takes a sequence of non-empty 1-D fp32 tensors")
        _need_gpu(w, _GPU_ONLY)
    dev = wavs[0].device
    wavs = [w.contiguous() for w in wavs]
    out = torch.empty((len(wavs), 2), dtype=torch.float32, device=dev)
    descs = (_capi.WtLevelClip * len(wavs))()
    for j, (d, w) in enumerate(zip(descs, wavs)):
        if w.device != dev:
            raise ValueError("level_many: the clips lie on different devices")
        d.x, d.n, d.out = w.data_ptr(), int(w.shape[0]), out.data_ptr() + 8 * j
    ws = torch.empty(int(lib.wt_level_workspace_bytes(len(wavs), sum(int(w.shape[0]) for w in wavs))), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.wt_level(descs, len(wavs), _ptr(ws), _stream(dev)), "wt_level")
    return out


def level(wav: torch.Tensor) -> torch.Tensor:
    """level_many for one clip (any shape: all its samples): (2,) fp32 = (peak, rms)."""
    return level_many([wav.reshape(-1)])[0]


def loudness_many(wavs: Sequence[torch.Tensor], sample_rate=24000, momentary: bool = False):
    """Integrated loudness of every clip (ITU-R BS.1770-4 / EBU R 128 as include/wavtokenizer_amd.h states it: K-weighting for
    the clip's rate, 400 ms blocks on a 100 ms grid, an absolute gate at -70 LUFS and a relative gate 10 LU under the mean).  wavs
    is a sequence of non-empty fp32 tensors on one GPU, (T,) or planar (C, T) with C <= 2 (channel weights 1.0); sample_rate is
    one rate or one per clip, each in [8000, 192000].  Returns (n, 3) fp32 there, row i = (L in LUFS, the relative threshold, the
    blocks through both gates); a clip shorter than 400 ms, silent or all of it under -70 LUFS reads (-inf, -inf, 0).
    momentary=True returns (that, [l_j (J_i,) fp32 per clip]), the loudness of every 400 ms block.  The clips are grouped by rate:
    one wt_loudness call (four launches) per rate.  The recurrence and the sums run in fp64 on the GPU; a clip has the same bits
    alone and in any batch.  Parity with pyloudnorm or ffmpeg is not pinned: neither was on hand to compare with."""
    wavs = list(wavs)
    if not wavs:
        raise ValueError("loudness_many takes at least one clip")
    if isinstance(sample_rate, (list, tuple)):
        rates = list(sample_rate)
        if len(rates) != len(wavs):
            raise ValueError("loudness_many: one sample rate per clip")
    else:
        rates = [sample_rate] * len(wavs)
    for r in rates:
        if isinstance(r, bool) or not isinstance(r, int) or not 8000 <= r <= 192000:
            raise ValueError("loudness_many: sample rates are ints in [8000, 192000]")
    for w in wavs:
        if (not isinstance(w, torch.Tensor) or w.dim() not in (1, 2) or w.shape[-1] < 1 or w.dtype != torch.float32
                or (w.dim() == 2 and w.shape[0] not in (1, 2))):
            raise ValueError("loudness_many takes a sequence of non-empty fp32 tensors (T,) or (C, T) with C <= 2")
    for w in wavs:
        _need_gpu(w, _GPU_ONLY)
    dev = wavs[0].device
    if any(w.device != dev for w in wavs):
        raise ValueError("loudness_many: the clips lie on different devices")
    wavs = [w.contiguous() for w in wavs]
    out = torch.empty((len(wavs), 3), dtype=torch.float32, device=dev)
    blocks: List[Optional[torch.Tensor]] = [None] * len(wavs)
    if momentary:
        counts = [int(lib.wt_loudness_blocks(int(w.shape[-1]), r)) for w, r in zip(wavs, rates)]
        flat = torch.empty(sum(counts), dtype=torch.float32, device=dev)
        pos = 0
        for i, c in enumerate(counts):
            blocks[i] = flat[pos:pos + c]
            pos += c
    with torch.cuda.device(dev):
        for rate in sorted(set(rates)):
            idx = [i for i, r in enumerate(rates) if r == rate]
            descs = (_capi.WtLoudnessClip * len(idx))()
            for d, i in zip(descs, idx):
                w = wavs[i]
                d.x, d.n, d.channels, d.channel_stride = w.data_ptr(), int(w.shape[-1]), (1 if w.dim() == 1 else int(w.shape[0])), int(w.shape[-1])
                d.out = out.data_ptr() + 12 * i
                d.blocks = blocks[i].data_ptr() if momentary and blocks[i].numel() else None
            ws = torch.empty(int(lib.wt_loudness_workspace_bytes(len(idx), sum(wavs[i].numel() for i in idx))), dtype=torch.uint8, device=dev)
            check(lib.wt_loudness(descs, len(idx), int(rate), _ptr(ws), _stream(dev)), "wt_loudness")
    return (out, blocks) if momentary else out


def loudness(wav: torch.Tensor, sample_rate: int = 24000) -> torch.Tensor:
    """loudness_many for one clip, (T,) or (C, T) with C <= 2: (3,) fp32 = (L in LUFS, relative threshold, gated blocks)."""
    return loudness_many([wav], sample_rate)[0]


def _r128_clips(who: str, wavs, sample_rate):
    """(clips made contiguous, their rates, their device) of a measuring call's arguments, checked as loudness_many checks them."""
    wavs = list(wavs)
    if not wavs:
        raise ValueError(who + " takes at least one clip")
    if isinstance(sample_rate, (list, tuple)):
        rates = list(sample_rate)
        if len(rates) != len(wavs):
            raise ValueError(who + ": one sample rate per clip")
    else:
        rates = [sample_rate] * len(wavs)
    for r in rates:
        if isinstance(r, bool) or not isinstance(r, int) or not 8000 <= r <= 192000:
            raise ValueError(who + ": sample rates are ints in [8000, 192000]")
    for w in wavs:
        if (not isinstance(w, torch.Tensor) or w.dim() not in (1, 2) or w.shape[-1] < 1 or w.dtype != torch.float32
                or (w.dim() == 2 and w.shape[0] not in (1, 2))):
            raise ValueError(who + " takes a sequence of non-empty fp32 tensors (T,) or (C, T) with C <= 2")
    for w in wavs:
        _need_gpu(w, _GPU_ONLY)
    dev = wavs[0].device
    if any(w.device != dev for w in wavs):
        raise ValueError(who + ": the clips lie on different devices")
    return [w.contiguous() for w in wavs], rates, dev


def _true_peak_linear(wavs, rates, dev) -> torch.Tensor:
    """(n, 2) fp32 on dev: (true peak, sample peak), linear; one wt_true_peak call per rate."""
    out = torch.empty((len(wavs), 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for rate in sorted(set(rates)):
            idx = [i for i, r in enumerate(rates) if r == rate]
            descs = (_capi.WtTruePeakClip * len(idx))()
            for d, i in zip(descs, idx):
                w = wavs[i]
                d.x, d.n, d.channels, d.channel_stride = w.data_ptr(), int(w.shape[-1]), (1 if w.dim() == 1 else int(w.shape[0])), int(w.shape[-1])
                d.out = out.data_ptr() + 8 * i
            ws = torch.empty(int(lib.wt_true_peak_workspace_bytes(len(idx), sum(wavs[i].numel() for i in idx))), dtype=torch.uint8, device=dev)
            check(lib.wt_true_peak(descs, len(idx), int(rate), _ptr(ws), _stream(dev)), "wt_true_peak")
    return out


def true_peak_many(wavs: Sequence[torch.Tensor], sample_rate=24000) -> torch.Tensor:
    """True peak of every clip by oversampling (ITU-R BS.1770-4 Annex 2 as include/wavtokenizer_amd.h states it: 4x under 96 kHz,
    2x under 192 kHz, a Hann-windowed sinc of 49 taps).  wavs and sample_rate as loudness_many takes them.  Returns (n, 2) fp32 on
    the clips' GPU, row i = (the true peak in dBTP, the sample peak in dBFS), both 20 log10 of the linear value (-inf for silence);
    the first is never below the second.  The clips are grouped by rate: one wt_true_peak call (two launches) per rate.  A maximum
    is exact: a clip has the same bits alone and in any batch.  Parity with libebur128 or ffmpeg is not pinned."""
    wavs, rates, dev = _r128_clips("true_peak_many", wavs, sample_rate)
    return 20.0 * torch.log10(_true_peak_linear(wavs, rates, dev))


def true_peak(wav: torch.Tensor, sample_rate: int = 24000) -> torch.Tensor:
    """true_peak_many for one clip, (T,) or (C, T) with C <= 2: (2,) fp32 = (dBTP, sample peak in dBFS)."""
    return true_peak_many([wav], sample_rate)[0]


def loudness_range_many(wavs: Sequence[torch.Tensor], sample_rate=24000, series: bool = False):
    """Integrated loudness, loudness range and the maxima of the momentary and the short-term loudness of every clip (EBU R 128 /
    Tech 3341 / Tech 3342 as include/wavtokenizer_amd.h states them: 3 s windows on the 100 ms grid, gates at -70 LUFS and 20 LU
    under the mean, the nearest-rank 10 % and 95 % points).  wavs and sample_rate as loudness_many takes them.  Returns (n, 9) fp32
    on the clips' GPU, row i = (L, the relative threshold, the gated blocks: the bits of loudness_many; LRA in LU, its low and its
    high value in LUFS, the windows through the range gates; the maximum momentary, the maximum short-term value).  A clip under
    3 s, silent or all of it under -70 LUFS has no range: (NaN, NaN, NaN, 0), and without a window a maximum short-term of -inf.
    series=True returns (that, [l_j (J_i,) per clip], [s_j (S_i,) per clip]): the momentary and the short-term loudness on the
    100 ms grid.  One wt_loudness_range call (four launches, one pass of the K-weighting) per rate; a clip has the same bits alone
    and in any batch."""
    wavs, rates, dev = _r128_clips("loudness_range_many", wavs, sample_rate)
    out = torch.empty((len(wavs), 9), dtype=torch.float32, device=dev)
    mom: List[Optional[torch.Tensor]] = [None] * len(wavs)
    sht: List[Optional[torch.Tensor]] = [None] * len(wavs)
    if series:
        nm = [int(lib.wt_loudness_blocks(int(w.shape[-1]), r)) for w, r in zip(wavs, rates)]
        ns = [int(lib.wt_short_term_blocks(int(w.shape[-1]), r)) for w, r in zip(wavs, rates)]
        flat = torch.empty(sum(nm) + sum(ns), dtype=torch.float32, device=dev)
        pos = 0
        for i, (a, b) in enumerate(zip(nm, ns)):
            mom[i], sht[i] = flat[pos:pos + a], flat[pos + a:pos + a + b]
            pos += a + b
    with torch.cuda.device(dev):
        for rate in sorted(set(rates)):
            idx = [i for i, r in enumerate(rates) if r == rate]
            descs = (_capi.WtLoudnessRangeClip * len(idx))()
            for d, i in zip(descs, idx):
                w = wavs[i]
                d.x, d.n, d.channels, d.channel_stride = w.data_ptr(), int(w.shape[-1]), (1 if w.dim() == 1 else int(w.shape[0])), int(w.shape[-1])
                d.out = out.data_ptr() + 36 * i
                d.momentary = mom[i].data_ptr() if series and mom[i].numel() else None
                d.short_term = sht[i].data_ptr() if series and sht[i].numel() else None
            ws = torch.empty(int(lib.wt_loudness_range_workspace_bytes(len(idx), sum(wavs[i].numel() for i in idx))), dtype=torch.uint8,
                             device=dev)
            check(lib.wt_loudness_range(descs, len(idx), int(rate), _ptr(ws), _stream(dev)), "wt_loudness_range")
    return (out, mom, sht) if series else out


def loudness_range(wav: torch.Tensor, sample_rate: int = 24000, series: bool = False):
    """loudness_range_many for one clip, (T,) or (C, T) with C <= 2: (9,) fp32; with series=True (that, l_j (J,), s_j (S,))."""
    if series:
        out, mom, sht = loudness_range_many([wav], sample_rate, series=True)
        return out[0], mom[0], sht[0]
    return loudness_range_many([wav], sample_rate)[0]


def r128_many(wavs: Sequence[torch.Tensor], sample_rate=24000) -> List[Dict[str, float]]:
    """What an R 128 meter's summary prints, per clip: {"integrated" (LUFS), "range" (LU), "range_low", "range_high" (LUFS),
    "true_peak" (dBTP), "sample_peak" (dBFS), "max_momentary", "max_short_term" (LUFS)} as Python floats, from one
    loudness_range_many and one true_peak_many (one transfer to the host)."""
    r = loudness_range_many(wavs, sample_rate)
    both = torch.cat([r, true_peak_many(wavs, sample_rate)], dim=1).cpu().tolist()
    return [{"integrated": v[0], "range": v[3], "range_low": v[4], "range_high": v[5], "true_peak": v[9], "sample_peak": v[10],
             "max_momentary": v[7], "max_short_term": v[8]} for v in both]


def normalize_args(who: str, normalize, target_db, target_lufs=None) -> Optional[Tuple[int, float]]:
    """The (mode, gain) of a call's normalize / target_db / target_lufs arguments, None without normalisation; for "lufs" the
    pair is (WT_NORM_LUFS, the target), -23.0 where target_lufs is None (not given).  ValueError, before any GPU work, for a mode other than "peak", "rms" and "lufs", for a
    target_db given without "peak" (the rms mode is Encodec's: it has no target), for a target_lufs given without "lufs", and for
    a target that is no finite number."""
    if isinstance(target_db, bool) or not isinstance(target_db, (int, float)) or not math.isfinite(target_db):
        raise ValueError(who + ": target_db must be a finite number")
    if target_lufs is not None:
        if isinstance(target_lufs, bool) or not isinstance(target_lufs, (int, float)) or not math.isfinite(target_lufs):
            raise ValueError(who + ": target_lufs must be a finite number")
        if normalize != "lufs":
            raise ValueError(who + ": target_lufs needs normalize='lufs'")
    if normalize is None:
        if target_db != 0.0:
            raise ValueError(who + ": target_db needs normalize='peak'")
        return None
    if normalize == "peak":
        return _capi.WT_NORM_PEAK, float(np.float32(10.0 ** (float(target_db) / 20.0)))
    if normalize == "rms" or normalize == "lufs":
        if target_db != 0.0:
            raise ValueError(who + ": target_db applies to normalize='peak' only")
        return (_capi.WT_NORM_RMS, 1.0) if normalize == "rms" else (_capi.WT_NORM_LUFS, -23.0 if target_lufs is None else float(target_lufs))
    raise ValueError(who + ": normalize must be None, 'peak', 'rms' or 'lufs'")


def ceiling_arg(who: str, normalize, max_true_peak_db) -> Optional[float]:
    """The true-peak ceiling of a call's max_true_peak_db argument as a float, None where it is not given.  ValueError, before any
    GPU work, for a ceiling that is no finite number (a bool is none) and for one given without normalize="lufs"."""
    if max_true_peak_db is None:
        return None
    if isinstance(max_true_peak_db, bool) or not isinstance(max_true_peak_db, (int, float)) or not math.isfinite(max_true_peak_db):
        raise ValueError(who + ": max_true_peak_db must be a finite number")
    if normalize != "lufs":
        raise ValueError(who + ": max_true_peak_db needs normalize='lufs'")
    return float(max_true_peak_db)


def normalize_rows(rows: torch.Tensor, n: Sequence[int], mode: int, gain: float, sample_rate: Optional[int] = None, *,
                   max_true_peak_db: Optional[float] = None) -> torch.Tensor:
    """wt_normalize_rows on rows, a contiguous (B, T_pad) fp32 tensor on the GPU, in place: row b's first n[b] samples are divided
    by their level (+ 1e-8); returns the divisors (B,) fp32.  mode WT_NORM_LUFS goes to wt_normalize_rows_lufs instead, gain then
    being the target in LUFS and sample_rate the rows' rate (the model's codec rate, for the tokenising calls), which that mode
    needs; with max_true_peak_db (dBTP, that mode only) to wt_normalize_rows_lufs_tp, which keeps every row's true peak under it."""
    if max_true_peak_db is not None:
        if mode != _capi.WT_NORM_LUFS:
            raise ValueError("normalize_rows: max_true_peak_db needs WT_NORM_LUFS")
        max_true_peak_db = ceiling_arg("normalize_rows", "lufs", max_true_peak_db)
    B, T_pad = rows.shape
    assert rows.dtype == torch.float32 and rows.is_contiguous() and len(n) == B
    dev = rows.device
    scales = torch.empty(B, dtype=torch.float32, device=dev)
    lens = (ctypes.c_int64 * B)(*[int(v) for v in n])
    if mode == _capi.WT_NORM_LUFS:
        if sample_rate is None:
            raise ValueError("normalize_rows: WT_NORM_LUFS needs the rows' sample_rate")
        if max_true_peak_db is not None:
            ws = torch.empty(int(lib.wt_normalize_rows_lufs_tp_workspace_bytes(B, T_pad)), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                check(lib.wt_normalize_rows_lufs_tp(_ptr(rows), B, T_pad, lens, int(sample_rate), float(gain), max_true_peak_db,
                                                    _ptr(scales), _ptr(ws), _stream(dev)), "wt_normalize_rows_lufs_tp")
            return scales
        ws = torch.empty(int(lib.wt_normalize_rows_lufs_workspace_bytes(B, T_pad)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib.wt_normalize_rows_lufs(_ptr(rows), B, T_pad, lens, int(sample_rate), float(gain), _ptr(scales), _ptr(ws),
                                             _stream(dev)), "wt_normalize_rows_lufs")
        return scales
    ws = torch.empty(int(lib.wt_normalize_rows_workspace_bytes(B, T_pad)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.wt_normalize_rows(_ptr(rows), B, T_pad, lens, int(mode), float(gain), _ptr(scales),
                                    _ptr(ws), _stream(dev)), "wt_normalize_rows")
    return scales


def normalize(wav: torch.Tensor, mode: str = "peak", target_db: float = 0.0, *, target_lufs: Optional[float] = None,
              sample_rate: int = 24000, max_true_peak_db: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-clip level normalisation of mono audio: wav is (T,), (B, T) or (B, 1, T) on the GPU; returns (wav / scale, scale), the
    first in wav's shape, scale (B,) fp32 (a 0-d tensor for (T,)).
      mode="peak": scale = max |x| + 1e-8, the bits of torch's fp32 x / (x.abs().max() + 1e-8) (extract_features.py:27-28); with
        target_db the quotient is multiplied by 10^(target_db / 20) rounded to fp32 (a peak target: -3 is the data preparation's).
      mode="rms":  scale = 1e-8 + sqrt(mean x^2), EncodecModel._encode_frame's (encoder/model.py:153-156).
      mode="lufs": scale = fp32(10^((L - target_lufs) / 20)), target_lufs -23.0 when not given, with L = loudness(x, sample_rate)[0], the integrated loudness (ITU-R
        BS.1770-4) at sample_rate, a rate in [8000, 192000]; the result then reads target_lufs.  A clip without a loudness
        (shorter than 400 ms, silent, or all of it under -70 LUFS) is returned as it is, bit for bit, with scale 1.  There is no
        limiter: a quiet clip with one loud click can exceed +-1 after the gain, unless max_true_peak_db (dBTP, "lufs" only) is
        given: the scale is then max(that, fp32(true peak / 10^(max_true_peak_db / 20))) with the true peak of true_peak(x,
        sample_rate), so that the result's true peak stays under the ceiling; a clip the ceiling does not bind has the bits of the
        call without it.  The ceiling bounds the gain of the whole clip; it is no sample-wise limiter.
    A silent clip stays zeros.  This is the one-clip definition the batched calls (encode_codes_many(normalize=...)) are compared
    with.  The audio is taken as it is: the reference's scripts normalise after convert_audio, sox's `norm` before the resampling,
    and a peak moves under resampling; parity with sox is not claimed, nor with pyloudnorm or ffmpeg for "lufs"."""
    args = normalize_args("normalize", mode, target_db, target_lufs)
    ceiling = ceiling_arg("normalize", mode, max_true_peak_db)
    if args is None:
        raise ValueError("normalize: mode must be 'peak', 'rms' or 'lufs'")
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or not 8000 <= sample_rate <= 192000:
        raise ValueError("normalize: sample_rate is an int in [8000, 192000]")
    if not isinstance(wav, torch.Tensor) or wav.dim() not in (1, 2, 3) or (wav.dim() == 3 and wav.shape[1] != 1) or wav.numel() < 1:
        raise ValueError("normalize takes non-empty mono audio (T,), (B, T) or (B, 1, T)")
    _need_gpu(wav, _GPU_ONLY)
    T = int(wav.shape[-1])
    rows = wav.to(torch.float32).reshape(-1, T).clone()
    scales = normalize_rows(rows, [T] * rows.shape[0], *args, sample_rate=sample_rate, max_true_peak_db=ceiling)
    return rows.view(wav.shape), (scales[0] if wav.dim() == 1 else scales)


def linear_overlap_add(frames: Sequence[torch.Tensor], stride: int) -> torch.Tensor:
    assert len(frames)
    _need_gpu(frames[0], _GPU_ONLY)
    dev = frames[0].device
    shape = frames[0].shape[:-1]
    flen, last = int(frames[0].shape[-1]), int(frames[-1].shape[-1])
    rows = 1
    for s in shape:
        rows *= int(s)
    buf = torch.zeros((len(frames), rows, flen), dtype=torch.float32, device=dev)
    for i, f in enumerate(frames):
        buf[i, :, : f.shape[-1]] = f.reshape(rows, -1)
    # the reference's triangle, from the same torch.linspace
    t = torch.linspace(0, 1, flen + 2, dtype=torch.float32)[1:-1]
    weight = (0.5 - (t - 0.5).abs()).to(dev)
    total = stride * (len(frames) - 1) + last
    out = torch.empty((rows, total), dtype=torch.float32, device=dev)
    check(lib.wt_linear_overlap_add(_ptr(buf), _ptr(weight), len(frames), rows, flen, last, int(stride), _ptr(out), _stream(dev)),
          "wt_linear_overlap_add")
    return out.view(*shape, total)


def segment_offsets(length: int, segment_length: int, stride: int) -> List[int]:
    """Offsets of the frames EncodecModel.encode cuts (encoder/model.py:139-145)."""
    return list(range(0, length, stride))


def segmented_round_trip(model, wav: torch.Tensor, segment_length: int, stride: int, bandwidth_id=None) -> torch.Tensor:
    """encode_infer + decode of a long clip in overlapping segments, cross-faded with the reference's linear
    overlap-add (EncodecModel.encode / .decode, encoder/model.py:122-190): wav [B, T] -> [B, T]."""
    _need_gpu(wav, _GPU_ONLY)
    bw = bandwidth_id if bandwidth_id is not None else torch.tensor([0])
    T = wav.shape[-1]
    outs = []
    for off in segment_offsets(T, segment_length, stride):
        frame = wav[..., off: off + segment_length]
        feats, _codes = model.encode_infer(frame, bandwidth_id=bw)
        outs.append(model.decode(feats, bandwidth_id=bw)[..., : frame.shape[-1]])
    return linear_overlap_add(outs, stride)[..., :T]
