"""The codec's evaluation metric on the GPU: log-mel spectrograms and their L1 distance, the reference's val/mel_loss
(MelSpecReconstructionLoss, decoder/loss.py:12-39, with safe_log, decoder/modules.py:194-205) as a number for inference users.

    mel_spectrogram(wav, ...)                 (T,), (B, T) or (B, 1, T) -> (..., n_mels, F), F = 1 + T // hop_length
    mel_spectrogram_many(wavs, ...)           clips of different lengths, one launch -> [(n_mels, F_i)] views of one flat tensor
    mel_distance(y_hat, y, ...)               0-dim: the mean of the per-clip distances (equal lengths: the reference's l1_loss mean)
    mel_distance_many(y_hats, ys, ...)        (n,) per-clip distances, one launch pair

The transform restates torchaudio.transforms.MelSpectrogram(sample_rate, n_fft=1024, hop_length=256, n_mels=100, center=True,
power=1) (include/wavtokenizer_amd.h gives the definition; parity with torchaudio itself is unpinned, it is not available to the
tests).  A clip's spectrogram and distance have the same bits alone, in any batch and at any position.  Tensors are fp32 on the
GPU; there is no CPU path.  `MelSpecReconstructionLoss()(y_hat, y)` becomes `mel_distance(y_hat, y)`.

And the intelligibility measure of the reference's evaluation script (metrics/infer.py:100-105, pystoi on the CPU per file):

    stoi(clean, processed, sample_rate, extended=False)          (T,) -> 0-dim; (B, T) or (B, 1, T) -> (B,)
    stoi_many(cleans, processeds, sample_rate=..., extended=False)   pairs of different lengths (and rates) -> (n,)

STOI (Taal et al. 2011) and, with extended=True, ESTOI (Jensen & Taal 2016), restated from the published algorithm
(include/wavtokenizer_amd.h gives the definition; parity with pystoi is unpinned, it is not available to the tests).  A pair's value
has the same bits alone, in any batch and at any position.  `stoi(raw, pre, sr, extended=False)` becomes `stoi(raw, pre, sr)`.

And the three measures that need no outside model and that codec papers report beside the mel distance:

    stft_distance(y_hat, y, fft_sizes=..., hop_sizes=..., win_lengths=..., components=False)   0-dim for (T,), else (B,)
    stft_distance_many(y_hats, ys, ...)       (n,); with components=True also (n, R, 2): per resolution (sc, mag)
    stft_magnitude(wav, n_fft, hop_length, win_length), stft_magnitude_many(wavs, ...)   the clamped |STFT|, (..., n_fft / 2 + 1, F)
    si_sdr(estimate, target, zero_mean=False), si_sdr_many(estimates, targets, ...)       dB, 0-dim for (T,), else (B,) / (n,)
    snr(estimate, target, zero_mean=False), snr_many(estimates, targets, ...)

The multi-resolution STFT distance of Parallel WaveGAN (spectral convergence + log-magnitude L1, the mean over the resolutions),
SI-SDR (Le Roux et al. 2019) and plain SNR, as include/wavtokenizer_amd.h defines them; parity with auraloss and torchmetrics is
unpinned, neither is available to the tests.  `MultiResolutionSTFTLoss()(x, y)` becomes `stft_distance(x, y)`,
`scale_invariant_signal_distortion_ratio(p, t)` becomes `si_sdr(p, t)` and `signal_noise_ratio(p, t)` becomes `snr(p, t)`.

And the periodicity family of the reference's evaluation script (metrics/periodicity.py, after cargan):

    pitch(wav, sample_rate=16000, threshold=0.15, silence_threshold=-60.0, unvoiced_threshold=0.5)   (T,) -> (f0 (n,), periodicity (n,))
    pitch_many(wavs, sample_rate=..., ...)    clips of different lengths (and rates) -> [(f0_i, periodicity_i)]
    periodicity_metrics(y, y_hat, sample_rate=16000, ...)         (T,) -> (3,): periodicity_loss, pitch_loss (cents), voiced/unvoiced F1
    periodicity_metrics_many(ys, y_hats, sample_rate=..., ...)    (n, 3)

The frame grid (1024 / 160 at 16 kHz, not centred), the A-weighted loudness gate and the three formulas are the reference's; the
pitch estimator is YIN (de Cheveigne & Kawahara 2002) where the reference runs CREPE, whose weights are not available here, so the
numbers are comparable between runs of this library and not with CREPE-based tables (include/wavtokenizer_amd.h gives the
definition, tests/pitch_ref.py holds it in float64).  `calculate_periodicity_metrics(y, y_hat)` becomes
`periodicity_metrics(y, y_hat, sample_rate)`.

And the level: loudness_delta(y_hat, y, sample_rate), loudness_delta_many(y_hats, ys, sample_rate=...), the difference of the
integrated loudness in LUFS (audio.loudness) of the decoded audio and its input, in LU; loudness_range_delta(_many) and
true_peak_delta(_many), the same differences of the loudness range (audio.loudness_range, LU) and of the true peak
(audio.true_peak, dB)."""
import ctypes
import math
from typing import Dict, List, Sequence, Tuple, Union

import torch

from ._capi import WtMelClip, WtPitchClip, WtPitchPair, WtStftdClip, WtStoiClip, WtWavedistClip, _need_gpu, _ptr, _stream, check, lib

_handles: Dict[Tuple[int, int, int, int, int], ctypes.c_void_p] = {}
_stoi_handles: Dict[Tuple[int, int], ctypes.c_void_p] = {}


_GPU_ONLY = ("wavtokenizer_amd.metrics runs only on an AMD GPU: move the tensor with .to('cuda'). "
             "There is no CPU path in this package.")


def mel_handle(sample_rate: int, n_fft: int, hop_length: int, n_mels: int, device_index: int) -> ctypes.c_void_p:
    """The wt_mel of a parameter set on a device, created once per process."""
    key = (int(sample_rate), int(n_fft), int(hop_length), int(n_mels), int(device_index))
    if key not in _handles:
        h = ctypes.c_void_p()
        check(lib.wt_mel_create(*key, ctypes.byref(h)), "wt_mel_create")
        _handles[key] = h
    return _handles[key]


def mel_frames(length: int, n_fft: int = 1024, hop_length: int = 256) -> int:
    """wt_mel_frames on the host: 1 + length // hop_length; ValueError for a clip reflect padding cannot take."""
    if int(length) <= n_fft // 2:
        raise ValueError(f"a clip of {int(length)} samples is too short for reflect padding by {n_fft // 2}")
    return 1 + int(length) // int(hop_length)


def _clips(who: str, wavs: Sequence[torch.Tensor]) -> Tuple[List[torch.Tensor], torch.device]:
    wavs = list(wavs)
    for w in wavs:
        if not isinstance(w, torch.Tensor) or w.dim() != 1:
            raise ValueError(who + ": every clip must be a 1-D tensor")
        _need_gpu(w, _GPU_ONLY)
    dev = wavs[0].device
    if any(w.device != dev for w in wavs):
        raise ValueError(who + ": all clips must be on one device")
    return [w.to(torch.float32).contiguous() for w in wavs], dev


def _rows(t: torch.Tensor, error: str) -> List[torch.Tensor]:
    """(T,), (B, T) or (B, 1, T) -> its rows as 1-D fp32 contiguous tensors; ValueError(error) for any other shape."""
    if t.dim() not in (1, 2, 3) or (t.dim() == 3 and t.shape[1] != 1):
        raise ValueError(error)
    return list(t.to(torch.float32).contiguous().view(-1, int(t.shape[-1])).unbind(0))


def _call(dev: torch.device, handle, workspace_bytes, call):
    """What the library calls here share: with dev current, handle(device index) is the table handle, workspace_bytes(handle)
    sizes the workspace, call(handle, workspace pointer, stream pointer) makes the call on the current stream."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(idx):
        h = handle(idx)
        ws = torch.empty((int(workspace_bytes(h)) + 7) // 8, dtype=torch.int64, device=dev)
        call(h, _ptr(ws), _stream(dev))
        # (the launches are queued on the current stream: the caching allocator hands ws and the inputs' copies out again only to
        # work queued behind them on that stream)


def _run(dev: torch.device, a: List[torch.Tensor], b, outs_numel: int, out_offsets: List[int], log, sample_rate, n_fft, hop_length, n_mels):
    """One wt_mel_spectrogram (b is None) or wt_mel_distance call over the clips; returns the flat output tensor."""
    n = len(a)
    frames = [mel_frames(w.shape[0], n_fft, hop_length) for w in a]
    out = torch.empty(outs_numel, dtype=torch.float32, device=dev)
    descs = (WtMelClip * n)()
    for i in range(n):
        descs[i].a = a[i].data_ptr()
        descs[i].b = b[i].data_ptr() if b is not None else None
        descs[i].length = a[i].shape[0]
        descs[i].out = out.data_ptr() + 4 * out_offsets[i]
    _call(dev, lambda idx: mel_handle(sample_rate, n_fft, hop_length, n_mels, idx),
          lambda h: lib.wt_mel_workspace_bytes(n, sum(frames) if b is not None else 0),
          lambda h, ws, stream: check(lib.wt_mel_spectrogram(h, descs, n, 1 if log else 0, ws, stream), "wt_mel_spectrogram") if b is None
          else check(lib.wt_mel_distance(h, descs, n, ws, stream), "wt_mel_distance"))
    return out, frames


def mel_spectrogram_many(wavs: Sequence[torch.Tensor], *, sample_rate: int = 24000, n_fft: int = 1024, hop_length: int = 256,
                         n_mels: int = 100, log: bool = True) -> List[torch.Tensor]:
    """Log-mel (log=False: linear mel) spectrograms of 1-D clips of different lengths in one launch: [(n_mels, F_i)], views of one
    flat tensor.  Clip i's result is the bits of mel_spectrogram(wavs[i])."""
    if not len(wavs):
        return []
    a, dev = _clips("mel_spectrogram_many", wavs)
    frames = [mel_frames(w.shape[0], n_fft, hop_length) for w in a]
    offs = [0]
    for f in frames:
        offs.append(offs[-1] + n_mels * f)
    flat, _ = _run(dev, a, None, offs[-1], offs[:-1], log, sample_rate, n_fft, hop_length, n_mels)
    return [flat[offs[i]: offs[i + 1]].view(n_mels, frames[i]) for i in range(len(a))]


def mel_spectrogram(wav: torch.Tensor, *, sample_rate: int = 24000, n_fft: int = 1024, hop_length: int = 256, n_mels: int = 100,
                    log: bool = True) -> torch.Tensor:
    """(T,), (B, T) or (B, 1, T) fp32 on the GPU -> (n_mels, F), (B, n_mels, F) or (B, 1, n_mels, F)."""
    _need_gpu(wav, _GPU_ONLY)
    a = _rows(wav, "mel_spectrogram: wav must be (T,), (B, T) or (B, 1, T)")
    F = mel_frames(wav.shape[-1], n_fft, hop_length)
    if not a:
        return torch.empty((*wav.shape[:-1], n_mels, F), dtype=torch.float32, device=wav.device)
    offs = [i * n_mels * F for i in range(len(a))]
    flat, _ = _run(wav.device, a, None, len(a) * n_mels * F, offs, log, sample_rate, n_fft, hop_length, n_mels)
    return flat.view(*wav.shape[:-1], n_mels, F)


def mel_distance_many(y_hats: Sequence[torch.Tensor], ys: Sequence[torch.Tensor], *, sample_rate: int = 24000, n_fft: int = 1024,
                      hop_length: int = 256, n_mels: int = 100) -> torch.Tensor:
    """Per pair of 1-D clips the mean of |log-mel(y_hat) - log-mel(y)| over the pair's n_mels * F entries: (n,) fp32, one launch
    pair for all clips.  The two clips of a pair must have one length (ValueError otherwise); pairs may differ."""
    y_hats, ys = list(y_hats), list(ys)
    if len(y_hats) != len(ys):
        raise ValueError("mel_distance_many: as many y_hats as ys")
    for i, (p, q) in enumerate(zip(y_hats, ys)):
        if isinstance(p, torch.Tensor) and isinstance(q, torch.Tensor) and p.dim() == 1 and q.dim() == 1 and p.shape[0] != q.shape[0]:
            raise ValueError(f"mel_distance_many: pair {i}: lengths {p.shape[0]} and {q.shape[0]} differ")
    if not y_hats:
        return torch.zeros(0, dtype=torch.float32, device="cuda")
    a, dev = _clips("mel_distance_many", y_hats)
    b, dev_b = _clips("mel_distance_many", ys)
    if dev_b != dev:
        raise ValueError("mel_distance_many: all clips must be on one device")
    out, _ = _run(dev, a, b, len(a), list(range(len(a))), True, sample_rate, n_fft, hop_length, n_mels)
    return out


def mel_distance(y_hat: torch.Tensor, y: torch.Tensor, *, sample_rate: int = 24000, n_fft: int = 1024, hop_length: int = 256,
                 n_mels: int = 100) -> torch.Tensor:
    """0-dim tensor: the mean over the clips of mel_distance_many's per-clip distances; y_hat and y are (T,), (B, T) or (B, 1, T)
    of one shape.  Every clip has the same number of entries, so this is the reference's l1_loss mean over the whole batch."""
    if y_hat.shape != y.shape:
        raise ValueError(f"mel_distance: shapes {tuple(y_hat.shape)} and {tuple(y.shape)} differ")
    p, q = (_rows(t, "mel_distance: inputs must be (T,), (B, T) or (B, 1, T)") for t in (y_hat, y))
    _need_gpu(y_hat, _GPU_ONLY)
    _need_gpu(y, _GPU_ONLY)
    return mel_distance_many(p, q, sample_rate=sample_rate, n_fft=n_fft, hop_length=hop_length, n_mels=n_mels).mean()


# ------------------------------------------------------------------------------------------------ STOI / ESTOI
STOI_FS = 10000


def stoi_ratio(sample_rate: int) -> Tuple[int, int]:
    """(p, q) = 10000 / sample_rate reduced; ValueError for a rate wt_stoi_create refuses (max(p, q) > 441)."""
    if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or int(sample_rate) < 1:
        raise ValueError(f"stoi: sample_rate must be a positive integer, not {sample_rate!r}")
    g = math.gcd(STOI_FS, int(sample_rate))
    p, q = STOI_FS // g, int(sample_rate) // g
    if max(p, q) > 441:
        raise ValueError(f"stoi: sample_rate {int(sample_rate)}: 10000 / sample_rate reduces to {p} / {q}, beyond 441 "
                         "(8, 10, 16, 22.05, 24, 32, 44.1 and 48 kHz are among the rates that work)")
    return p, q


def stoi_frames(length: int, sample_rate: int) -> Tuple[int, int]:
    """(samples at 10 kHz, candidate frames K0) of a clip; ValueError for a clip too short for one frame."""
    p, q = stoi_ratio(sample_rate)
    n = -(-int(length) * p // q)
    if n <= 256:
        raise ValueError(f"stoi: a clip of {int(length)} samples at {int(sample_rate)} Hz has {n} samples at 10 kHz: one frame needs "
                         "more than 256")
    return n, (n - 256 + 127) // 128


def stoi_handle(sample_rate: int, device_index: int) -> ctypes.c_void_p:
    """The wt_stoi of a rate on a device, created once per process."""
    key = (int(sample_rate), int(device_index))
    if key not in _stoi_handles:
        h = ctypes.c_void_p()
        check(lib.wt_stoi_create(*key, ctypes.byref(h)), "wt_stoi_create")
        _stoi_handles[key] = h
    return _stoi_handles[key]


def _stoi_run(dev: torch.device, a: List[torch.Tensor], b: List[torch.Tensor], sample_rate: int, extended: bool, out: torch.Tensor,
              slots: Sequence[int]):
    """One wt_stoi call: pair i's value goes to out[slots[i]]."""
    n = len(a)
    sizes = [stoi_frames(w.shape[0], sample_rate) for w in a]
    descs = (WtStoiClip * n)()
    for i in range(n):
        descs[i].clean = a[i].data_ptr()
        descs[i].processed = b[i].data_ptr()
        descs[i].length = a[i].shape[0]
        descs[i].out = out.data_ptr() + 4 * slots[i]
    _call(dev, lambda idx: stoi_handle(sample_rate, idx),
          lambda h: lib.wt_stoi_workspace_bytes(h, n, sum(s[0] for s in sizes), sum(s[1] for s in sizes)),
          lambda h, ws, stream: check(lib.wt_stoi(h, descs, n, 1 if extended else 0, ws, stream, None), "wt_stoi"))


def stoi_many(cleans: Sequence[torch.Tensor], processeds: Sequence[torch.Tensor], *, sample_rate: Union[int, Sequence[int]] = 24000,
              extended: bool = False) -> torch.Tensor:
    """STOI (extended=True: ESTOI) of pairs of 1-D clips: (n,) fp32, one call per sample rate for all the pairs of that rate.
    sample_rate is one rate or one per pair (any sequence, numpy array or tensor of integers).  The two clips of a pair must have one length (ValueError otherwise); pairs may
    differ.  Pair i's value is the bits of stoi(cleans[i], processeds[i], rate_i)."""
    cleans, processeds = list(cleans), list(processeds)
    if len(cleans) != len(processeds):
        raise ValueError("stoi_many: as many cleans as processeds")
    if hasattr(sample_rate, "tolist"):          # a numpy array or a tensor of rates, or a 0-dim one or a numpy scalar: one rate
        sample_rate = sample_rate.tolist()
    if isinstance(sample_rate, Sequence) and not isinstance(sample_rate, (str, bytes)):
        rates = list(sample_rate)
        if len(rates) != len(cleans):
            raise ValueError("stoi_many: one sample_rate, or one per pair")
    else:
        rates = [sample_rate] * len(cleans)
    for r in set(rates):
        stoi_ratio(r)
    for i, (p, q) in enumerate(zip(cleans, processeds)):
        if isinstance(p, torch.Tensor) and isinstance(q, torch.Tensor) and p.dim() == 1 and q.dim() == 1:
            if p.shape[0] != q.shape[0]:
                raise ValueError(f"stoi_many: pair {i}: lengths {p.shape[0]} and {q.shape[0]} differ")
            stoi_frames(p.shape[0], rates[i])
    if not cleans:
        return torch.zeros(0, dtype=torch.float32, device="cuda")
    a, dev = _clips("stoi_many", cleans)
    b, dev_b = _clips("stoi_many", processeds)
    if dev_b != dev:
        raise ValueError("stoi_many: all clips must be on one device")
    out = torch.empty(len(a), dtype=torch.float32, device=dev)
    for r in sorted(set(int(r) for r in rates)):
        sel = [i for i, ri in enumerate(rates) if int(ri) == r]
        _stoi_run(dev, [a[i] for i in sel], [b[i] for i in sel], r, bool(extended), out, sel)
    return out


def stoi(clean: torch.Tensor, processed: torch.Tensor, sample_rate: int = 24000, extended: bool = False) -> torch.Tensor:
    """STOI (extended=True: ESTOI) of processed against clean, both at sample_rate: (T,) gives a 0-dim tensor, (B, T) and (B, 1, T)
    give (B,), one value per row."""
    if clean.shape != processed.shape:
        raise ValueError(f"stoi: shapes {tuple(clean.shape)} and {tuple(processed.shape)} differ")
    p, q = (_rows(t, "stoi: inputs must be (T,), (B, T) or (B, 1, T)") for t in (clean, processed))
    stoi_frames(clean.shape[-1], sample_rate)
    _need_gpu(clean, _GPU_ONLY)
    _need_gpu(processed, _GPU_ONLY)
    d = stoi_many(p, q, sample_rate=int(sample_rate), extended=extended) if p else torch.zeros(0, dtype=torch.float32, device=clean.device)
    return d[0] if clean.dim() == 1 else d


# ------------------------------------------------------------------------------------------------ pairs of clips
def _pairs(who: str, first: Sequence[torch.Tensor], second: Sequence[torch.Tensor], longer_than: int = 0):
    """Two lists of 1-D clips as fp32 contiguous tensors on one device, pair i of one length above longer_than: ValueError otherwise."""
    first, second = list(first), list(second)
    if len(first) != len(second):
        raise ValueError(who + ": as many estimates as targets")
    for i, (p, q) in enumerate(zip(first, second)):
        if isinstance(p, torch.Tensor) and isinstance(q, torch.Tensor) and p.dim() == 1 and q.dim() == 1 and p.shape[0] != q.shape[0]:
            raise ValueError(f"{who}: pair {i}: lengths {p.shape[0]} and {q.shape[0]} differ")
        if isinstance(p, torch.Tensor) and p.dim() == 1 and p.shape[0] <= longer_than:
            raise ValueError(f"{who}: pair {i}: a clip of {p.shape[0]} samples is too short: more than {longer_than} are needed")
    if not first:
        return [], [], None
    a, dev = _clips(who, first)
    b, dev_b = _clips(who, second)
    if dev_b != dev:
        raise ValueError(who + ": all clips must be on one device")
    return a, b, dev


def _batch(who: str, first: torch.Tensor, second: torch.Tensor):
    """(T,), (B, T) or (B, 1, T) tensors of one shape -> their rows."""
    if first.shape != second.shape:
        raise ValueError(f"{who}: shapes {tuple(first.shape)} and {tuple(second.shape)} differ")
    p, q = (_rows(t, who + ": inputs must be (T,), (B, T) or (B, 1, T)") for t in (first, second))
    _need_gpu(first, _GPU_ONLY)
    _need_gpu(second, _GPU_ONLY)
    return p, q


# ------------------------------------------------------------------------------------------------ multi-resolution STFT distance
STFT_FFT_SIZES, STFT_HOP_SIZES, STFT_WIN_LENGTHS = (1024, 2048, 512), (120, 240, 50), (600, 1200, 240)
_stftd_handles: Dict[Tuple, ctypes.c_void_p] = {}


def stft_resolutions(fft_sizes=STFT_FFT_SIZES, hop_sizes=STFT_HOP_SIZES, win_lengths=STFT_WIN_LENGTHS) -> Tuple[Tuple[int, int, int], ...]:
    """The resolutions (n_fft, hop, win_length) of a parameter set, checked: ValueError for anything wt_stftd_create refuses."""
    try:
        sets = [tuple(int(v) for v in x) for x in (fft_sizes, hop_sizes, win_lengths)]
    except TypeError:
        raise ValueError("stft_distance: fft_sizes, hop_sizes and win_lengths are sequences of integers") from None
    if not (len(sets[0]) == len(sets[1]) == len(sets[2])) or not 1 <= len(sets[0]) <= 8:
        raise ValueError("stft_distance: fft_sizes, hop_sizes and win_lengths need one length, between 1 and 8")
    res = tuple(zip(*sets))
    for n_fft, hop, win in res:
        if n_fft not in (512, 1024, 2048):
            raise ValueError(f"stft_distance: n_fft {n_fft}: must be 512, 1024 or 2048")
        if not 1 <= hop <= n_fft or not 1 <= win <= n_fft:
            raise ValueError(f"stft_distance: hop {hop} and win_length {win} must lie in 1..n_fft = {n_fft}")
    return res


def stft_frames(length: int, n_fft: int, hop_length: int) -> int:
    """wt_stftd_frames on the host: 1 + length // hop_length; ValueError for a clip reflect padding cannot take."""
    if int(length) <= n_fft // 2:
        raise ValueError(f"a clip of {int(length)} samples is too short for reflect padding by {n_fft // 2}")
    return 1 + int(length) // int(hop_length)


def stftd_handle(resolutions: Tuple[Tuple[int, int, int], ...], device_index: int) -> ctypes.c_void_p:
    """The wt_stftd of a set of resolutions on a device, created once per process."""
    key = (tuple(resolutions), int(device_index))
    if key not in _stftd_handles:
        n = len(resolutions)
        arrays = [(ctypes.c_int32 * n)(*[r[i] for r in resolutions]) for i in range(3)]
        h = ctypes.c_void_p()
        check(lib.wt_stftd_create(n, *arrays, int(device_index), ctypes.byref(h)), "wt_stftd_create")
        _stftd_handles[key] = h
    return _stftd_handles[key]


def _stftd_descs(a: List[torch.Tensor], b, out: torch.Tensor, offsets: Sequence[int]):
    descs = (WtStftdClip * len(a))()
    for i in range(len(a)):
        descs[i].estimate = a[i].data_ptr()
        descs[i].target = b[i].data_ptr() if b is not None else None
        descs[i].length = a[i].shape[0]
        descs[i].out = out.data_ptr() + 4 * offsets[i]
    return descs


def stft_distance_many(y_hats: Sequence[torch.Tensor], ys: Sequence[torch.Tensor], *, fft_sizes=STFT_FFT_SIZES, hop_sizes=STFT_HOP_SIZES,
                       win_lengths=STFT_WIN_LENGTHS, components: bool = False):
    """The multi-resolution STFT distance of pairs of 1-D clips (estimate, target): (n,) fp32, one launch per resolution and one
    more for all pairs.  With components=True also (n, R, 2): per resolution the spectral convergence and the log-magnitude L1; the
    distance is their fp32 sum over the resolutions in order, divided by R.  The two clips of a pair must have one length
    (ValueError otherwise), more than max(fft_sizes) // 2 samples; pairs may differ."""
    res = stft_resolutions(fft_sizes, hop_sizes, win_lengths)
    R = len(res)
    need = max(r[0] for r in res)
    a, b, dev = _pairs("stft_distance_many", y_hats, ys, need // 2)
    frames = [sum(stft_frames(w.shape[0], need, r[1]) for r in res) for w in a]
    if not a:
        empty = torch.zeros(0, dtype=torch.float32, device="cuda")
        return (empty, empty.view(0, R, 2)) if components else empty
    n, width = len(a), 1 + 2 * R
    out = torch.empty((n, width), dtype=torch.float32, device=dev)
    descs = _stftd_descs(a, b, out, [i * width for i in range(n)])
    _call(dev, lambda idx: stftd_handle(res, idx), lambda h: lib.wt_stftd_workspace_bytes(h, n, sum(frames)),
          lambda h, ws, stream: check(lib.wt_stftd_distance(h, descs, n, ws, stream), "wt_stftd_distance"))
    return (out[:, 0], out[:, 1:].view(n, R, 2)) if components else out[:, 0]


def stft_distance(y_hat: torch.Tensor, y: torch.Tensor, *, fft_sizes=STFT_FFT_SIZES, hop_sizes=STFT_HOP_SIZES,
                  win_lengths=STFT_WIN_LENGTHS, components: bool = False):
    """y_hat and y are (T,), (B, T) or (B, 1, T) of one shape: (T,) gives a 0-dim tensor, the others (B,), one distance per row
    (their mean is MultiResolutionSTFTLoss's batch value up to the order of its sums).  components=True: also (R, 2) or (B, R, 2)."""
    res = stft_resolutions(fft_sizes, hop_sizes, win_lengths)
    p, q = _batch("stft_distance", y_hat, y)
    stft_frames(y.shape[-1], max(r[0] for r in res), 1)
    if not p:
        d, c = torch.zeros(0, dtype=torch.float32, device=y.device), torch.zeros((0, len(res), 2), dtype=torch.float32, device=y.device)
    else:
        d, c = stft_distance_many(p, q, fft_sizes=fft_sizes, hop_sizes=hop_sizes, win_lengths=win_lengths, components=True)
    if y.dim() == 1:
        d, c = d[0], c[0]
    return (d, c) if components else d


def stft_magnitude_many(wavs: Sequence[torch.Tensor], n_fft: int = 1024, hop_length: int = 120, win_length: int = 600) -> List[torch.Tensor]:
    """The clamped STFT magnitudes sqrt(max(re^2 + im^2, 1e-7)) of 1-D clips of different lengths at one resolution in one launch:
    [(n_fft / 2 + 1, F_i)], views of one flat tensor: what the distance is made of, bit for bit."""
    res = stft_resolutions((n_fft,), (hop_length,), (win_length,))
    if not len(wavs):
        return []
    a, dev = _clips("stft_magnitude_many", wavs)
    bins = res[0][0] // 2 + 1
    frames = [stft_frames(w.shape[0], res[0][0], res[0][1]) for w in a]
    offs = [0]
    for f in frames:
        offs.append(offs[-1] + bins * f)
    flat = torch.empty(offs[-1], dtype=torch.float32, device=dev)
    descs = _stftd_descs(a, None, flat, offs[:-1])
    n = len(a)
    _call(dev, lambda idx: stftd_handle(res, idx), lambda h: lib.wt_stftd_workspace_bytes(h, n, 0),
          lambda h, ws, stream: check(lib.wt_stftd_magnitude(h, 0, descs, n, ws, stream), "wt_stftd_magnitude"))
    return [flat[offs[i]: offs[i + 1]].view(bins, frames[i]) for i in range(n)]


def stft_magnitude(wav: torch.Tensor, n_fft: int = 1024, hop_length: int = 120, win_length: int = 600) -> torch.Tensor:
    """(T,), (B, T) or (B, 1, T) fp32 on the GPU -> (bins, F), (B, bins, F) or (B, 1, bins, F), bins = n_fft / 2 + 1."""
    res = stft_resolutions((n_fft,), (hop_length,), (win_length,))
    a = _rows(wav, "stft_magnitude: wav must be (T,), (B, T) or (B, 1, T)")
    bins, F = res[0][0] // 2 + 1, stft_frames(wav.shape[-1], res[0][0], res[0][1])
    _need_gpu(wav, _GPU_ONLY)
    if not a:
        return torch.empty((*wav.shape[:-1], bins, F), dtype=torch.float32, device=wav.device)
    outs = stft_magnitude_many(a, n_fft, hop_length, win_length)
    return torch.stack(outs).view(*wav.shape[:-1], bins, F)


# ------------------------------------------------------------------------------------------------ SI-SDR and SNR
def wavedist_many(estimates: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], *, zero_mean: bool = False,
                  who: str = "wavedist_many") -> torch.Tensor:
    """One wt_wavedist call over pairs of 1-D clips: (n, 2) fp32, per pair (SI-SDR, SNR) in dB."""
    a, b, dev = _pairs(who, estimates, targets, 0)
    if not a:
        return torch.zeros((0, 2), dtype=torch.float32, device="cuda")
    n = len(a)
    out = torch.empty((n, 2), dtype=torch.float32, device=dev)
    descs = (WtWavedistClip * n)()
    for i in range(n):
        descs[i].estimate, descs[i].target, descs[i].length = a[i].data_ptr(), b[i].data_ptr(), a[i].shape[0]
        descs[i].out = out.data_ptr() + 8 * i
    total = sum(w.shape[0] for w in a)
    _call(dev, lambda idx: None, lambda h: lib.wt_wavedist_workspace_bytes(n, total),
          lambda h, ws, stream: check(lib.wt_wavedist(descs, n, 1 if zero_mean else 0, ws, stream), "wt_wavedist"))
    return out


def si_sdr_many(estimates: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], *, zero_mean: bool = False) -> torch.Tensor:
    """The scale-invariant signal-to-distortion ratio in dB of pairs of 1-D clips: (n,) fp32.  The two clips of a pair must have one
    length (ValueError otherwise); pairs may differ.  zero_mean=True first takes each signal's own mean off."""
    return wavedist_many(estimates, targets, zero_mean=zero_mean, who="si_sdr_many")[:, 0]


def snr_many(estimates: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], *, zero_mean: bool = False) -> torch.Tensor:
    """The signal-to-noise ratio in dB of pairs of 1-D clips (estimate, target): (n,) fp32; si_sdr_many's rules."""
    return wavedist_many(estimates, targets, zero_mean=zero_mean, who="snr_many")[:, 1]


def _wavedist(who: str, column: int, estimate: torch.Tensor, target: torch.Tensor, zero_mean: bool) -> torch.Tensor:
    if estimate.shape == target.shape and estimate.dim() >= 1 and estimate.shape[-1] < 1:
        raise ValueError(who + ": the signals are empty")
    p, q = _batch(who, estimate, target)
    d = wavedist_many(p, q, zero_mean=zero_mean, who=who)[:, column] if p else torch.zeros(0, dtype=torch.float32, device=target.device)
    return d[0] if target.dim() == 1 else d


def si_sdr(estimate: torch.Tensor, target: torch.Tensor, zero_mean: bool = False) -> torch.Tensor:
    """SI-SDR in dB of estimate against target: (T,) gives a 0-dim tensor, (B, T) and (B, 1, T) give (B,), one value per row."""
    return _wavedist("si_sdr", 0, estimate, target, zero_mean)


def snr(estimate: torch.Tensor, target: torch.Tensor, zero_mean: bool = False) -> torch.Tensor:
    """SNR in dB of estimate against target: (T,) gives a 0-dim tensor, (B, T) and (B, 1, T) give (B,), one value per row."""
    return _wavedist("snr", 1, estimate, target, zero_mean)


# ------------------------------------------------------------------------------------------------ pitch, periodicity, voiced / unvoiced F1
PITCH_RATE, PITCH_WINDOW, PITCH_HOP = 16000, 1024, 160
_pitch_handles: Dict[int, ctypes.c_void_p] = {}


def pitch_frames(length: int) -> int:
    """wt_pitch_frames on the host: 1 + (length - 1024) // 160 frames of a clip of `length` samples at 16 kHz, 0 below 1024."""
    return 0 if int(length) < PITCH_WINDOW else 1 + (int(length) - PITCH_WINDOW) // PITCH_HOP


def pitch_handle(device_index: int) -> ctypes.c_void_p:
    """The wt_pitch of a device, created once per process."""
    key = int(device_index)
    if key not in _pitch_handles:
        h = ctypes.c_void_p()
        check(lib.wt_pitch_create(key, ctypes.byref(h)), "wt_pitch_create")
        _pitch_handles[key] = h
    return _pitch_handles[key]


def _pitch_rates(who: str, sample_rate, n: int) -> List[int]:
    """One rate per clip from one rate or a sequence of them; ValueError for anything but positive integers."""
    if hasattr(sample_rate, "tolist"):
        sample_rate = sample_rate.tolist()
    rates = list(sample_rate) if isinstance(sample_rate, Sequence) and not isinstance(sample_rate, (str, bytes)) else [sample_rate] * n
    if len(rates) != n:
        raise ValueError(who + ": one sample_rate, or one per clip")
    for r in rates:
        if isinstance(r, bool) or int(r) != r or int(r) < 1:
            raise ValueError(f"{who}: sample_rate must be a positive integer, not {r!r}")
    return [int(r) for r in rates]


def _pitch_check(who: str, clips: Sequence[torch.Tensor], rates: List[int]) -> None:
    """What can be refused before any GPU work: integer samples (the loudness gate needs the scale of floating-point audio in
    -1..1: PCM would pass it shifted by 90 dB), a clip too short for one frame at 16 kHz, a rate pair the resampler refuses."""
    from . import audio
    for i, (w, r) in enumerate(zip(clips, rates)):
        if isinstance(w, torch.Tensor) and not w.is_floating_point():
            raise ValueError(f"{who}: clip {i}: dtype {w.dtype}: the clips must be floating-point audio")
        if isinstance(w, torch.Tensor) and w.dim() == 1:
            n = w.shape[0] if r == PITCH_RATE else audio.resampled_length(r, PITCH_RATE, w.shape[0])
            if n < PITCH_WINDOW:
                raise ValueError(f"{who}: clip {i}: a clip of {w.shape[0]} samples at {r} Hz is too short: one frame needs "
                                 f"{PITCH_WINDOW} samples at 16 kHz")


def _pitch_at_16k(clips: List[torch.Tensor], rates: List[int]) -> List[torch.Tensor]:
    """The clips at 16 kHz: a clip at another rate goes through the project's own resampler, as audio.convert_audio(clip, sr, 16000)."""
    from . import audio
    return [w if r == PITCH_RATE else audio.convert_audio(w.view(1, -1), r, PITCH_RATE)[0].contiguous() for w, r in zip(clips, rates)]


def _pitch_thresholds(who: str, threshold, silence_threshold, unvoiced_threshold) -> Tuple[float, float, float]:
    t = tuple(float(v) for v in (threshold, silence_threshold, unvoiced_threshold))
    if any(math.isnan(v) for v in t):
        raise ValueError(who + ": a threshold is NaN")
    return t


def pitch_many(wavs: Sequence[torch.Tensor], *, sample_rate: Union[int, Sequence[int]] = PITCH_RATE, threshold: float = 0.15,
               silence_threshold: float = -60.0, unvoiced_threshold: float = 0.5) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """Pitch and periodicity tracks of 1-D clips of different lengths (and rates) in one call: [(f0_i, periodicity_i)], each (n_i,)
    fp32 with n_i = pitch_frames(length at 16 kHz), views of one flat tensor; the bits of pitch(wavs[i], rate_i).  See pitch."""
    wavs = list(wavs)
    rates = _pitch_rates("pitch_many", sample_rate, len(wavs))
    thr = _pitch_thresholds("pitch_many", threshold, silence_threshold, unvoiced_threshold)
    _pitch_check("pitch_many", wavs, rates)
    if not wavs:
        return []
    a, dev = _clips("pitch_many", wavs)
    a = _pitch_at_16k(a, rates)
    n = len(a)
    frames = [pitch_frames(w.shape[0]) for w in a]
    offs = [0]
    for f in frames:
        offs.append(offs[-1] + 2 * f)
    flat = torch.empty(offs[-1], dtype=torch.float32, device=dev)
    descs = (WtPitchClip * n)()
    for i in range(n):
        descs[i].signal, descs[i].length, descs[i].out, descs[i].taps = a[i].data_ptr(), a[i].shape[0], flat.data_ptr() + 4 * offs[i], None
    _call(dev, pitch_handle, lambda h: lib.wt_pitch_workspace_bytes(n, sum(frames)),
          lambda h, ws, stream: check(lib.wt_pitch_track(h, descs, n, *thr, ws, stream), "wt_pitch_track"))
    return [(flat[offs[i]: offs[i] + frames[i]], flat[offs[i] + frames[i]: offs[i + 1]]) for i in range(n)]


def pitch(wav: torch.Tensor, sample_rate: int = PITCH_RATE, *, threshold: float = 0.15, silence_threshold: float = -60.0,
          unvoiced_threshold: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """(f0, periodicity) of a 1-D clip, each (n,) fp32: per frame of 1024 samples at a hop of 160 at 16 kHz (not centred: n = 1 +
    (T - 1024) // 160; a clip at another rate is first resampled with this package's resampler) the YIN estimate of the pitch in Hz
    within 50..550 Hz and 1 - d' at its lag, a periodicity in 0..1.  A frame whose A-weighted loudness is under silence_threshold dB
    has its periodicity set to 0, and a frame whose periodicity is under unvoiced_threshold is unvoiced: its f0 is NaN.  threshold
    is YIN's absolute threshold on d'.  The reference's predict_pitch has these roles with CREPE as the estimator and
    unvoiced_threshold 0.21, which is calibrated for CREPE's confidence; for YIN, 1 - d' is approximately the normalised
    autocorrelation at the period, and the default here is 0.5."""
    if not isinstance(wav, torch.Tensor) or wav.dim() != 1:
        raise ValueError("pitch: wav must be a 1-D tensor")
    return pitch_many([wav], sample_rate=sample_rate, threshold=threshold,
                      silence_threshold=silence_threshold, unvoiced_threshold=unvoiced_threshold)[0]


def periodicity_metrics_many(ys: Sequence[torch.Tensor], y_hats: Sequence[torch.Tensor], *, sample_rate: Union[int, Sequence[int]] = PITCH_RATE,
                             threshold: float = 0.15, silence_threshold: float = -60.0, unvoiced_threshold: float = 0.5) -> torch.Tensor:
    """The reference's calculate_periodicity_metrics(y, y_hat) per pair of 1-D clips (reference, estimate): (n, 3) fp32, per pair the
    periodicity RMSE, the pitch RMSE in cents over the frames voiced in both (NaN without one) and the voiced / unvoiced F1 (NaN
    where precision or recall is 0 / 0, as the reference's, which its caller filters with math.isnan), on the tracks of pitch();
    one call for all pairs.  The two clips of a pair must have one length (ValueError otherwise); pairs may differ in length and
    rate.  The estimator is YIN, not the reference's CREPE: comparable between runs of this library, not with CREPE-based tables."""
    ys, y_hats = list(ys), list(y_hats)
    rates = _pitch_rates("periodicity_metrics_many", sample_rate, len(ys))
    thr = _pitch_thresholds("periodicity_metrics_many", threshold, silence_threshold, unvoiced_threshold)
    if len(ys) == len(y_hats):
        _pitch_check("periodicity_metrics_many", ys, rates)
        _pitch_check("periodicity_metrics_many", y_hats, rates)
    a, b, dev = _pairs("periodicity_metrics_many", ys, y_hats, 0)
    if not a:
        return torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    a, b = _pitch_at_16k(a, rates), _pitch_at_16k(b, rates)
    n = len(a)
    frames = [pitch_frames(w.shape[0]) for w in a]
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    descs = (WtPitchPair * n)()
    for i in range(n):
        descs[i].reference, descs[i].estimate, descs[i].length, descs[i].out = a[i].data_ptr(), b[i].data_ptr(), a[i].shape[0], out.data_ptr() + 12 * i
    _call(dev, pitch_handle, lambda h: lib.wt_pitch_workspace_bytes(n, sum(frames)),
          lambda h, ws, stream: check(lib.wt_pitch_pairs(h, descs, n, *thr, ws, stream), "wt_pitch_pairs"))
    return out


def periodicity_metrics(y: torch.Tensor, y_hat: torch.Tensor, sample_rate: int = PITCH_RATE, *, threshold: float = 0.15,
                        silence_threshold: float = -60.0, unvoiced_threshold: float = 0.5) -> torch.Tensor:
    """(3,) fp32: periodicity_loss, pitch_loss in cents and the voiced / unvoiced F1 of the estimate y_hat against the reference y,
    two 1-D clips of one length at sample_rate.  See periodicity_metrics_many and pitch."""
    for t in (y, y_hat):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError("periodicity_metrics: y and y_hat must be 1-D tensors")
    return periodicity_metrics_many([y], [y_hat], sample_rate=sample_rate, threshold=threshold, silence_threshold=silence_threshold,
                                    unvoiced_threshold=unvoiced_threshold)[0]


# ---- loudness: did the decoded audio keep the level of the input? -------------------------------------------------------------
def loudness_delta_many(y_hats: Sequence[torch.Tensor], ys: Sequence[torch.Tensor], *, sample_rate: Union[int, Sequence[int]] = 24000) -> torch.Tensor:
    """L(y_hat) - L(y) in LU per pair, L the integrated loudness of audio.loudness (ITU-R BS.1770-4 / EBU R 128; include/
    wavtokenizer_amd.h gives the definition, parity with pyloudnorm is unpinned): (n,) fp32.  The clips are fp32 on the GPU, (T,) or
    planar (C, T) with C <= 2; the two of a pair share a rate (sample_rate: one, or one per pair) and may differ in length.  One
    audio.loudness_many call over both lists.  NaN where either side has no loudness (under 400 ms, silent, all under -70 LUFS)."""
    from . import audio
    y_hats, ys = list(y_hats), list(ys)
    if len(y_hats) != len(ys):
        raise ValueError("loudness_delta_many: as many estimates as references")
    if not ys:
        raise ValueError("loudness_delta_many takes at least one pair")
    if isinstance(sample_rate, (list, tuple)):
        if len(sample_rate) != len(ys):
            raise ValueError("loudness_delta_many: one sample rate per pair")
        sample_rate = list(sample_rate) * 2
    L = audio.loudness_many(y_hats + ys, sample_rate)[:, 0]
    a, b = L[:len(ys)], L[len(ys):]
    return torch.where(torch.isinf(a) | torch.isinf(b), torch.full_like(a, float("nan")), a - b)


def loudness_delta(y_hat: torch.Tensor, y: torch.Tensor, sample_rate: int = 24000) -> torch.Tensor:
    """0-dim fp32: loudness_delta_many for one pair."""
    return loudness_delta_many([y_hat], [y], sample_rate=sample_rate)[0]


def _paired(who: str, y_hats, ys, sample_rate):
    """(y_hats + ys, the rates of that list) of a delta call's arguments."""
    y_hats, ys = list(y_hats), list(ys)
    if len(y_hats) != len(ys):
        raise ValueError(who + ": as many estimates as references")
    if not ys:
        raise ValueError(who + " takes at least one pair")
    if isinstance(sample_rate, (list, tuple)):
        if len(sample_rate) != len(ys):
            raise ValueError(who + ": one sample rate per pair")
        sample_rate = list(sample_rate) * 2
    return y_hats + ys, sample_rate


def loudness_range_delta_many(y_hats: Sequence[torch.Tensor], ys: Sequence[torch.Tensor], *,
                              sample_rate: Union[int, Sequence[int]] = 24000) -> torch.Tensor:
    """LRA(y_hat) - LRA(y) in LU per pair, LRA the loudness range of audio.loudness_range (EBU Tech 3342 on the 100 ms grid;
    include/wavtokenizer_amd.h gives the definition): (n,) fp32.  Arguments as loudness_delta_many takes them.  One
    audio.loudness_range_many call over both lists.  NaN where either side has no range (under 3 s, silent, all under -70 LUFS)."""
    from . import audio
    both, rates = _paired("loudness_range_delta_many", y_hats, ys, sample_rate)
    r = audio.loudness_range_many(both, rates)[:, 3]
    return r[:len(both) // 2] - r[len(both) // 2:]


def loudness_range_delta(y_hat: torch.Tensor, y: torch.Tensor, sample_rate: int = 24000) -> torch.Tensor:
    """0-dim fp32: loudness_range_delta_many for one pair."""
    return loudness_range_delta_many([y_hat], [y], sample_rate=sample_rate)[0]


def true_peak_delta_many(y_hats: Sequence[torch.Tensor], ys: Sequence[torch.Tensor], *,
                         sample_rate: Union[int, Sequence[int]] = 24000) -> torch.Tensor:
    """dBTP(y_hat) - dBTP(y) in dB per pair, the true peak of audio.true_peak (ITU-R BS.1770-4 Annex 2): (n,) fp32.  Arguments as
    loudness_delta_many takes them.  One audio.true_peak_many call over both lists.  NaN where either side is silent."""
    from . import audio
    both, rates = _paired("true_peak_delta_many", y_hats, ys, sample_rate)
    t = audio.true_peak_many(both, rates)[:, 0]
    a, b = t[:len(both) // 2], t[len(both) // 2:]
    return torch.where(torch.isinf(a) | torch.isinf(b), torch.full_like(a, float("nan")), a - b)


def true_peak_delta(y_hat: torch.Tensor, y: torch.Tensor, sample_rate: int = 24000) -> torch.Tensor:
    """0-dim fp32: true_peak_delta_many for one pair."""
    return true_peak_delta_many([y_hat], [y], sample_rate=sample_rate)[0]
