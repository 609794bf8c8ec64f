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
has the same bits alone, in any batch and at any position.  `stoi(raw, pre, sr, extended=False)` becomes `stoi(raw, pre, sr)`."""
import ctypes
import math
from typing import Dict, List, Sequence, Tuple, Union

import torch

from ._capi import WtMelClip, WtStoiClip, _need_gpu, _ptr, _stream, check, lib

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
