"""Definitions, bounds and C-ABI wrappers for the R 128 meter kernels (csrc/r128.hip: wt_true_peak, wt_loudness_range,
wt_normalize_rows_lufs_tp): tests/test_r128_host.py, test_true_peak_op.py, test_loudness_range_op.py and test_r128_calls.py share
them.  K-weighting, lufs, bound and the clip makers are tests/loudness_ref.py's.

The three definitions are those of include/wavtokenizer_amd.h, here in float64 with numpy:
  true peak: the 49-tap Hann-windowed sinc rounded to fp32 (the taps the device uses), the interpolation itself in float64;
  short-term loudness: 3 s windows on the 100 ms grid of the loudness section, complete windows only, no gate;
  loudness range: gates at -70 LUFS and 20 LU under the mean of the absolutely gated, the nearest-rank 10 % and 95 % points.
Bounds.  True peak: (48 / F + 1) * 2^-24 * max_p sum_k |h[p + F k]| * max |x|, the standard bound of a 48 / F-term fp32 dot
product.  Short-term and range values: loudness_ref.bound, the error of the same definition through a sequential fp32 lfilter."""
import ctypes
import math

import numpy as np
import torch

from tests import loudness_ref as R

SENTINEL = R.SENTINEL
WINDOW = 30                        # 100 ms segments in a short-term window


# ---- true peak -----------------------------------------------------------------------------------------------------------------
def factor(fs: int) -> int:
    return 4 if fs < 96000 else 2 if fs < 192000 else 1


def taps(F: int) -> np.ndarray:
    """h[0..48] in double, rounded to fp32."""
    j = np.arange(49, dtype=np.float64)
    return (np.sinc((j - 24.0) / F) * 0.5 * (1.0 - np.cos(2.0 * np.pi * j / 48.0))).astype(np.float32)


def true_peak(x, fs: int, F: int = None):
    """(true peak, sample peak, bound) of x, (n,) or (C, n): linear, in float64 on the fp32 taps; bound is what an fp32 evaluation
    of any interpolated value may differ from float64 by.  F: the oversampling factor where it is not to be the rate's."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    F = factor(fs) if F is None else F
    sp = float(np.abs(x).max())
    if F == 1:
        return sp, sp, 0.0
    h = taps(F).astype(np.float64)
    H, T = 24 // F, 48 // F
    tp, norm1 = sp, 0.0
    for p in range(1, F):
        g = h[p:48:F]
        assert g.shape[0] == T
        norm1 = max(norm1, float(np.abs(g).sum()))
        for ch in x:
            y = np.convolve(ch, g)[H:H + ch.shape[0]]          # y[i] = sum_k g[k] x[i + H - k], zeros outside the clip
            tp = max(tp, float(np.abs(y).max()))
    return tp, sp, (T + 1) * 2.0 ** -24 * norm1 * sp


def db(v: float) -> float:
    return 20.0 * math.log10(v) if v > 0 else -math.inf


# ---- short-term loudness and loudness range ---------------------------------------------------------------------------------------
def short_term_blocks(n: int, fs: int) -> int:
    """Complete 3 s windows: the j >= 0 with floor((j + 30) fs / 10) <= n."""
    j = 0
    while (j + WINDOW) * fs // 10 <= n:
        j += 1
    return j


def ranks(m: int):
    """The nearest-rank 10 % and 95 % points among m sorted values, in integer arithmetic."""
    return ((m - 1) + 5) // 10, (19 * (m - 1) + 10) // 20


def select(z_sorted: np.ndarray):
    lo, hi = ranks(len(z_sorted))
    return z_sorted[lo], z_sorted[hi]


def short_term(x, fs: int, dtype=np.float64, y=None):
    """(z_j, s_j) of the S windows of x, (n,) or (C, n); dtype is the filter's arithmetic, sums are float64; with y (C, n), the
    K-weighted channels are taken from there."""
    x = np.atleast_2d(np.asarray(x))
    n = x.shape[1]
    S = short_term_blocks(n, fs)
    z = np.zeros(S, np.float64)
    if S == 0:
        return z, R.lufs(z)
    y = R.weighted(x, fs, dtype) if y is None else y
    assert y.shape == x.shape
    edges = np.array([j * fs // 10 for j in range(S + WINDOW)], dtype=np.int64)
    for ch in range(x.shape[0]):
        q = y[ch].astype(np.float64) ** 2
        seg = np.add.reduceat(q[:edges[-1]], edges[:-1])
        win = np.convolve(seg, np.ones(WINDOW), "valid")        # 30 terms each (no running sum: a quiet window after loud ones would cancel)
        z += win[:S] / (edges[WINDOW:] - edges[:-WINDOW])[:S]
    return z, R.lufs(z)


def loudness_range(z: np.ndarray):
    """(LRA, low, high, m, relative gate, margin) of the window energies z: margin is the least distance of a window from either
    range gate in LU (inf without a finite window)."""
    s = R.lufs(z)
    keep = s > -70.0
    fin = s[np.isfinite(s)]
    margin = float(np.abs(fin + 70.0).min()) if fin.size else math.inf
    if not keep.any():
        return math.nan, math.nan, math.nan, 0, -math.inf, margin
    rel = float(R.lufs(z[keep].mean())) - 20.0
    margin = min(margin, float(np.abs(fin - rel).min()))
    keep &= s > rel
    m = int(keep.sum())
    if m == 0:
        return math.nan, math.nan, math.nan, 0, rel, margin
    z_lo, z_hi = select(np.sort(z[keep]))
    lo, hi = float(R.lufs(z_lo)), float(R.lufs(z_hi))
    return hi - lo, lo, hi, m, rel, margin


def tone_levels(levels_db, seconds: float = 20.0, fs: int = 48000) -> np.ndarray:
    """Two channels of a 1 kHz tone, `seconds` at each level in dBFS: the signals of Tech 3342's cases."""
    n = int(seconds * fs)
    t = np.arange(n * len(levels_db)) / fs
    amp = np.repeat([10.0 ** (d / 20.0) for d in levels_db], n)
    ch = amp * np.sin(2 * np.pi * 1000.0 * t)
    return np.stack([ch, ch])


def make_stepped(n: int, fs: int, seed: int, levels_db, step_s: float = 1.0) -> np.ndarray:
    """n fp32 samples of white noise whose level steps through levels_db (standard deviation in dBFS), step_s seconds each,
    cyclically."""
    rng = np.random.default_rng(seed)
    step = int(step_s * fs)
    idx = (np.arange(n) // step) % len(levels_db)
    amp = (10.0 ** (np.asarray(levels_db, dtype=np.float64) / 20.0))[idx]
    return (rng.standard_normal(n) * amp).astype(np.float32)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _describe(d, c):
    assert c.dtype == torch.float32 and c.dim() in (1, 2) and c.stride(-1) == 1
    d.x, d.n, d.channels = c.data_ptr(), c.shape[-1], (1 if c.dim() == 1 else c.shape[0])
    d.channel_stride = c.stride(0) if c.dim() == 2 else 0
    return d.n * d.channels


def measure_true_peak(clips, fs: int) -> np.ndarray:
    """One wt_true_peak over clips (fp32 views on the GPU, (n,) or (C, n) with unit sample stride): (B, 2) fp32 on the CPU, linear;
    checks that nothing is written behind the workspace or the results."""
    from wavtokenizer_amd import _capi
    B = len(clips)
    out = torch.full((B + 1, 2), SENTINEL, dtype=torch.float32, device="cuda")
    descs = (_capi.WtTruePeakClip * B)()
    total = 0
    for j, (d, c) in enumerate(zip(descs, clips)):
        total += _describe(d, c)
        d.out = out.data_ptr() + 8 * j
    nbytes = int(_capi.lib.wt_true_peak_workspace_bytes(B, total))
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(_capi.lib.wt_true_peak(descs, B, fs, ctypes.c_void_p(ws.data_ptr()), _stream()), "wt_true_peak")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xAB).all()), "wt_true_peak wrote behind its workspace"
    assert bool((out[B] == SENTINEL).all()), "wt_true_peak wrote behind its results"
    return out[:B].cpu().numpy()


def measure_range(clips, fs: int, series: bool = True):
    """One wt_loudness_range over clips: ((B, 9) fp32 on the CPU, [l_j per clip], [s_j per clip]); checks that nothing is written
    behind the workspace, the results or either series (with series=False: that neither series is touched)."""
    from wavtokenizer_amd import _capi
    B = len(clips)
    out = torch.full((B + 1, 9), SENTINEL, dtype=torch.float32, device="cuda")
    Js = [int(_capi.lib.wt_loudness_blocks(c.shape[-1], fs)) for c in clips]
    Ss = [int(_capi.lib.wt_short_term_blocks(c.shape[-1], fs)) for c in clips]
    mom = [torch.full((J + 2,), SENTINEL, dtype=torch.float32, device="cuda") for J in Js]
    sht = [torch.full((S + 2,), SENTINEL, dtype=torch.float32, device="cuda") for S in Ss]
    descs = (_capi.WtLoudnessRangeClip * B)()
    total = 0
    for j, (d, c) in enumerate(zip(descs, clips)):
        total += _describe(d, c)
        d.out = out.data_ptr() + 36 * j
        d.momentary, d.short_term = (mom[j].data_ptr(), sht[j].data_ptr()) if series else (None, None)
    nbytes = int(_capi.lib.wt_loudness_range_workspace_bytes(B, total))
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(_capi.lib.wt_loudness_range(descs, B, fs, ctypes.c_void_p(ws.data_ptr()), _stream()), "wt_loudness_range")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xAB).all()), "wt_loudness_range wrote behind its workspace"
    assert bool((out[B] == SENTINEL).all()), "wt_loudness_range wrote behind its results"
    for count, arrs in ((Js, mom), (Ss, sht)):
        for k, a in zip(count, arrs):
            assert bool((a[k:] == SENTINEL).all()) and (series or bool((a == SENTINEL).all())), "wt_loudness_range wrote behind a series"
    return out[:B].cpu().numpy(), [a[:k].cpu().numpy() for k, a in zip(Js, mom)], [a[:k].cpu().numpy() for k, a in zip(Ss, sht)]


def normalize_rows_lufs_tp(rows, n, fs: int, target: float, ceiling_db: float):
    """wt_normalize_rows_lufs_tp in place on rows (B, T_pad) fp32 on the GPU; returns the scales (B,)."""
    from wavtokenizer_amd import _capi
    B, T_pad = rows.shape
    scales = torch.full((B + 1,), -7.0, dtype=torch.float32, device="cuda")
    nbytes = int(_capi.lib.wt_normalize_rows_lufs_tp_workspace_bytes(B, T_pad))
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(_capi.lib.wt_normalize_rows_lufs_tp(ctypes.c_void_p(rows.data_ptr()), B, T_pad, (ctypes.c_int64 * B)(*n), fs, target,
                                                    ceiling_db, ctypes.c_void_p(scales.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                                    _stream()), "wt_normalize_rows_lufs_tp")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xAB).all()), "wt_normalize_rows_lufs_tp wrote behind its workspace"
    assert float(scales[B]) == -7.0, "wt_normalize_rows_lufs_tp wrote behind the scales"
    return scales[:B]
