"""The multi-resolution STFT distance of csrc/stftd.hip (include/wavtokenizer_amd.h gives the definition) in float64 numpy, two fp32
stand-ins that serve as yardsticks for the kernels' rounding error (a plain radix-2 FFT for the magnitudes per bin; torch.stft in
fp32 on the CPU with fp32 sums for the distance values), the error statistic, and the signals and ctypes plumbing the tests share.
Written from the definition (what auraloss.freq.MultiResolutionSTFTLoss computes with its defaults); auraloss is not available
here, so the parity with it is unpinned."""
import functools

import numpy as np

from tests.mel_ref import Arena, Outputs

FLOOR = 1e-7
EPS32 = 2.0 ** -23
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))       # (n_fft, hop, win_length): the Parallel WaveGAN set


def window64(n_fft: int, win: int):
    """The periodic Hann window of win samples, zero-padded to n_fft with (n_fft - win) // 2 zeros on the left, in float64.  One
    sample: the window [1.], as torch.hann_window(1) gives (the formula alone would give [0.])."""
    w = np.zeros(n_fft, np.float64)
    left = (n_fft - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win) if win > 1 else 1.0
    return w


def n_frames(T: int, hop: int) -> int:
    return 1 + T // hop


def frame_index(T: int, n_fft: int, hop: int):
    """[F][n_fft] indices into the reflect-padded clip."""
    return np.arange(n_frames(T, hop))[:, None] * hop + np.arange(n_fft)[None, :]


def frames64(x, n_fft: int, hop: int, win: int):
    """The windowed frames [F][n_fft] of a clip in float64: reflect padding by n_fft / 2, frame f starts at f * hop."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 1 and x.shape[0] > n_fft // 2
    xp = np.pad(x, n_fft // 2, mode="reflect")
    return xp[frame_index(x.shape[0], n_fft, hop)] * window64(n_fft, win)[None, :]


def magnitude64(x, n_fft: int, hop: int, win: int):
    """(S [bins][F], norms [F]): the clamped magnitudes in float64 and the 2-norm of every windowed frame."""
    fr = frames64(x, n_fft, hop, win)
    X = np.fft.rfft(fr, axis=1)
    S = np.sqrt(np.maximum(X.real ** 2 + X.imag ** 2, FLOOR))
    return S.T, np.sqrt((fr * fr).sum(axis=1))


def distance64(x, y, resolutions=RESOLUTIONS):
    """(distance, [R][2] (sc_r, mag_r)) of estimate x against target y in float64."""
    comps = []
    for n_fft, hop, win in resolutions:
        X, Y = magnitude64(x, n_fft, hop, win)[0], magnitude64(y, n_fft, hop, win)[0]
        comps.append((np.sqrt(((Y - X) ** 2).sum()) / np.sqrt((Y ** 2).sum()), np.abs(np.log(Y) - np.log(X)).mean()))
    comps = np.asarray(comps, np.float64)
    return float(comps.sum(axis=1).mean()), comps


def _bitrev(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])


def standin_magnitude_fp32(x, n_fft: int, hop: int, win: int):
    """The magnitudes in float32 throughout with a plain radix-2 decimation-in-time complex FFT of the n_fft windowed samples (zero
    imaginary part): window and twiddles rounded once from float64, every product and sum rounded to float32.  [bins][F] float32."""
    f32 = np.float32
    x = np.asarray(x, f32)
    xp = np.pad(x, n_fft // 2, mode="reflect")
    F = n_frames(x.shape[0], hop)
    re = (xp[frame_index(x.shape[0], n_fft, hop)] * window64(n_fft, win).astype(f32)[None, :])[:, _bitrev(n_fft)].astype(f32)
    im = np.zeros_like(re)
    half = 1
    while half < n_fft:
        ang = -np.pi * np.arange(half, dtype=np.float64) / half
        wr, wi = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
        re = re.reshape(F, -1, 2, half)
        im = im.reshape(F, -1, 2, half)
        tr = (re[:, :, 1] * wr - im[:, :, 1] * wi).astype(f32)
        ti = (re[:, :, 1] * wi + im[:, :, 1] * wr).astype(f32)
        re = np.stack([re[:, :, 0] + tr, re[:, :, 0] - tr], axis=2).astype(f32).reshape(F, n_fft)
        im = np.stack([im[:, :, 0] + ti, im[:, :, 0] - ti], axis=2).astype(f32).reshape(F, n_fft)
        half *= 2
    bins = n_fft // 2 + 1
    power = (re[:, :bins] * re[:, :bins] + im[:, :bins] * im[:, :bins]).astype(f32)
    return np.sqrt(np.maximum(power, f32(FLOOR))).astype(f32).T


def standin_distance_fp32(x, y, resolutions=RESOLUTIONS):
    """(distance, [R][2]) in fp32 on the CPU: torch.stft of fp32 signals, clamp, sqrt, norms, log and mean, every sum in fp32."""
    import torch
    x, y = torch.from_numpy(np.asarray(x, np.float32)), torch.from_numpy(np.asarray(y, np.float32))
    comps = []
    for n_fft, hop, win in resolutions:
        w = torch.hann_window(win, periodic=True, dtype=torch.float32)
        mags = []
        for s in (x, y):
            Z = torch.stft(s, n_fft, hop_length=hop, win_length=win, window=w, center=True, pad_mode="reflect", return_complex=True)
            mags.append(torch.sqrt(torch.clamp(Z.real ** 2 + Z.imag ** 2, min=FLOOR)))
        X, Y = mags
        sc = torch.sqrt(((Y - X) ** 2).sum()) / torch.sqrt((Y ** 2).sum())
        mg = (torch.log(Y) - torch.log(X)).abs().mean()
        comps.append((float(sc), float(mg)))
    comps = np.asarray(comps, np.float64)
    return float(np.float32(np.float32(comps.sum(axis=1).astype(np.float32).sum()) / np.float32(len(resolutions)))), comps


def error_stat(S, S64, norms) -> float:
    """r = max |S - S64| / (2^-23 (||w x_f||_2 + S64)): FFT rounding is relative to the frame's energy, not to the bin."""
    err = np.abs(np.asarray(S, np.float64) - S64)
    return float((err / (EPS32 * (norms[None, :] + S64))).max())


def total_fp32(comps) -> np.float32:
    """out[0] from the components as stftd_reduce_block forms it: the fp32 sum of (sc_r + mag_r) over r in order, over n_res."""
    f32 = np.float32
    t = f32(0)
    for sc, mg in np.asarray(comps, f32):
        t = f32(t + f32(sc + mg))
    return f32(t / f32(len(comps)))


# ------------------------------------------------------------------------------------------------ signals
SIGNALS = ("noise", "noise_tone", "tone", "impulse", "dc", "quiet")
BROADBAND = ("noise", "noise_tone", "quiet", "impulse")


def signal(name: str, T: int, seed: int = 0, sample_rate: int = 24000):
    rng = np.random.default_rng(1000 * seed + T)
    t = np.arange(T, dtype=np.float64) / sample_rate
    if name == "noise":
        x = 0.1 * rng.standard_normal(T)
    elif name == "noise_tone":
        x = 0.1 * rng.standard_normal(T) + 0.5 * np.sin(2 * np.pi * 440.0 * t)
    elif name == "tone":
        x = 0.5 * np.sin(2 * np.pi * 440.0 * t)
    elif name == "impulse":
        x = np.zeros(T)
        x[T // 3] = 0.5
    elif name == "dc":
        x = np.full(T, 0.25)
    elif name == "quiet":
        x = 1e-3 * rng.standard_normal(T)
    elif name == "silence":
        x = np.zeros(T)
    else:
        raise KeyError(name)
    return x.astype(np.float32)


def estimate_of(name: str, target):
    """The estimate that goes with a broadband target in the distance checks: the target at 0.8 plus a fifth of its level of
    fresh noise (the impulse: at 0.8, and a smaller one seven samples later)."""
    T = len(target)
    if name == "impulse":
        x = 0.8 * target.astype(np.float64)
        x[T // 3 + 7] += 0.05
        return x.astype(np.float32)
    level = {"noise": 0.1, "noise_tone": 0.1, "quiet": 1e-3}[name]
    return (0.8 * target + 0.2 * level * np.random.default_rng(77 + T).standard_normal(T)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the calls, through ctypes
@functools.lru_cache(maxsize=None)
def handle(resolutions=RESOLUTIONS):
    from wavtokenizer_amd import metrics
    return metrics.stftd_handle(tuple(resolutions), 0)


def run_magnitude(clips, n_fft, hop, win, ws_fill=0xAB):
    """One wt_stftd_magnitude call on clips laid out in a NaN arena, outputs between canaries.  ([bins][F] arrays, canaries intact)."""
    import ctypes

    import torch

    from wavtokenizer_amd._capi import WtStftdClip, check, lib
    n = len(clips)
    arena = Arena(list(clips))
    bins = n_fft // 2 + 1
    F = [n_frames(len(c), hop) for c in clips]
    outs = Outputs([bins * f for f in F])
    h = handle(((n_fft, hop, win),))
    nbytes = int(lib.wt_stftd_workspace_bytes(h, n, 0))
    ws = torch.full((nbytes + 64,), ws_fill, dtype=torch.uint8, device="cuda")
    descs = (WtStftdClip * n)()
    for i in range(n):
        descs[i].estimate, descs[i].target, descs[i].length, descs[i].out = arena.ptr(i), None, len(clips[i]), outs.ptr(i)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.wt_stftd_magnitude(h, 0, descs, n, ctypes.c_void_p(ws.data_ptr()), stream), "wt_stftd_magnitude")
    torch.cuda.synchronize()
    got, intact = outs.read()
    assert bool((ws[nbytes:] == ws_fill).all()), "the call wrote behind its workspace"
    return [g.reshape(bins, f) for g, f in zip(got, F)], intact


def run_distance(estimates, targets, resolutions=RESOLUTIONS, ws_fill=0xAB):
    """One wt_stftd_distance call on pairs laid out in a NaN arena, outputs between canaries, the workspace filled with ws_fill
    beforehand.  ([1 + 2 R] float32 arrays, canaries intact)."""
    import ctypes

    import torch

    from wavtokenizer_amd._capi import WtStftdClip, check, lib
    n = len(estimates)
    arena = Arena(list(estimates) + list(targets))
    width = 1 + 2 * len(resolutions)
    outs = Outputs([width] * n)
    h = handle(tuple(resolutions))
    total = sum(n_frames(len(c), hop) for c in estimates for _n, hop, _w in resolutions)
    nbytes = int(lib.wt_stftd_workspace_bytes(h, n, total))
    ws = torch.full((nbytes + 64,), ws_fill, dtype=torch.uint8, device="cuda")
    descs = (WtStftdClip * n)()
    for i in range(n):
        descs[i].estimate, descs[i].target, descs[i].length, descs[i].out = arena.ptr(i), arena.ptr(n + i), len(estimates[i]), outs.ptr(i)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.wt_stftd_distance(h, descs, n, ctypes.c_void_p(ws.data_ptr()), stream), "wt_stftd_distance")
    torch.cuda.synchronize()
    got, intact = outs.read()
    assert bool((ws[nbytes:] == ws_fill).all()), "the call wrote behind its workspace"
    return got, intact
