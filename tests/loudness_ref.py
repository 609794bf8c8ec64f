"""Definition, bounds and C-ABI wrappers for the loudness kernels (csrc/loudness.hip: wt_loudness, wt_normalize_rows_lufs):
tests/test_loudness_host.py, test_loudness_op.py, test_loudness_calls.py and test_loudness_rates.py share them.

The definition is ITU-R BS.1770-4 / EBU R 128 integrated loudness as include/wavtokenizer_amd.h states it, here in float64 with
scipy.signal.lfilter and numpy: K-weighting (two biquads, coefficients computed for the clip's integer rate), blocks of 400 ms on a
100 ms grid in integer arithmetic (complete blocks only), an absolute gate at -70 LUFS and a relative gate 10 LU under the mean of
the blocks that passed the first.

The bound the GPU is held to is the error of the SAME definition evaluated with a sequential fp32 lfilter (fp32 coefficients,
fp32 state, the squares summed in float64) against float64, or two fp32 ulps of the result where that is larger (the result is
stored as fp32: half an ulp is spent on that alone).  The device runs the recurrence in fp64 and is expected far inside.

A second, tighter bound (bound64; tests/test_loudness_rates.py) takes the fp32 lfilter out of it: two fp32 ulps plus four times
the distance between the definition and a float64 stand-in of the device's chunked evaluation (weighted_chunked), measured per
clip.  Where the fp32 lfilter is off by 10^-2 LU (content under the high pass at 96 kHz and above), that distance is 10^-7."""
import ctypes
import math

import numpy as np
import torch
from scipy.signal import lfilter

RATES = (8000, 11025, 16000, 22050, 24000, 44100, 48000, 96000, 192000)


def kweight(fs: int):
    """((b, a) of the high shelf, (b, a) of the high pass) in float64 for the integer rate fs."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    high = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return shelf, high


def coefficients10(fs: int) -> np.ndarray:
    """b0 b1 b2 a1 a2 of the shelf, then of the high pass: the layout of wt_kweight_coefficients."""
    (b1, a1), (b2, a2) = kweight(fs)
    return np.concatenate([b1, a1[1:], b2, a2[1:]])


def blocks(n: int, fs: int) -> int:
    """Complete 400 ms blocks: the j >= 0 with floor((j + 4) fs / 10) <= n."""
    j = 0
    while (j + 4) * fs // 10 <= n:
        j += 1
    return j


def lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def weighted(x, fs: int, dtype=np.float64) -> np.ndarray:
    """The K-weighted channels of x, (n,) or (C, n) with C <= 2, as (C, n): a sequential lfilter in dtype."""
    x = np.atleast_2d(np.asarray(x))
    assert x.shape[0] in (1, 2)
    (b1, a1), (b2, a2) = kweight(fs)
    out = []
    for ch in x:
        y = lfilter(b1.astype(dtype), a1.astype(dtype), ch.astype(dtype))
        y = lfilter(b2.astype(dtype), a2.astype(dtype), y.astype(dtype))
        assert y.dtype == dtype
        out.append(y)
    return np.stack(out)


def _step(c, s, x):
    """One sample through both biquads (transposed direct form II) for every column: s (4, K) moves on, the weighted samples return."""
    y1 = c[0] * x + s[0]
    s[0] = c[1] * x + s[1] - c[3] * y1
    s[1] = c[2] * x - c[4] * y1
    y2 = c[5] * y1 + s[2]
    s[2] = c[6] * y1 + s[3] - c[8] * y2
    s[3] = c[7] * y1 - c[9] * y2
    return y2


def weighted_chunked(x, fs: int, chunk: int) -> np.ndarray:
    """The K-weighted channels of x as (C, n) in float64, evaluated the way the device orders the work, not the way the definition
    reads: every chunk of `chunk` samples is walked from zero state; the end states z_k go through s_{k+1} = M s_k + z_k,
    M = A^chunk, by a log-step scan with M^(2^i) inside groups of 64 chunks, the groups' totals are chained with M^64, the start
    state of chunk 64 g + l is M^l carry_g + the scan's value of its left neighbour; then every chunk is walked again from its
    start state.  Plain numpy products and sums (no fused multiply-add), all chunks of a channel at once: its distance from the
    sequential float64 lfilter is what the reordering alone costs in float64 (bound64)."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    assert x.shape[0] in (1, 2) and chunk >= 1 and chunk & (chunk - 1) == 0
    c = coefficients10(fs)
    A = np.zeros((4, 4))
    for j in range(4):
        s = np.zeros((4, 1))
        s[j] = 1.0
        _step(c, s, np.zeros(1))
        A[:, j] = s[:, 0]
    M = A
    for _ in range(chunk.bit_length() - 1):
        M = M @ M
    P = [M]
    for _ in range(6):
        P.append(P[-1] @ P[-1])                                 # P[i] = M^(2^i); P[6] = M^64
    n = x.shape[1]
    K = -(-n // chunk)
    G = -(-K // 64)
    out = []
    for ch in x:
        xs = np.zeros(G * 64 * chunk)
        xs[:n] = ch
        xs = xs.reshape(G * 64, chunk).T                        # (chunk, chunks): one row per step of the walk
        s = np.zeros((4, G * 64))
        for t in range(chunk):
            _step(c, s, xs[t])
        s[:, K:] = 0.0                                          # (chunks past the clip carry nothing)
        z = s.T.reshape(G, 64, 4).copy()
        for i in range(6):
            d = 1 << i
            z[:, d:] = z[:, :-d] @ P[i].T + z[:, d:]
        carry = np.zeros((G, 4))
        run = np.zeros(4)
        for g in range(G):
            carry[g] = run
            run = P[6] @ run + z[g, 63]
        v = np.repeat(carry[:, None, :], 64, axis=1)            # M^l carry_g, l in binary
        lane = np.arange(64)
        for i in range(6):
            bit = ((lane >> i) & 1).astype(bool)
            v[:, bit] = v[:, bit] @ P[i].T
        v[:, 1:] += z[:, :-1]
        s = v.reshape(G * 64, 4).T.copy()
        y = np.empty((chunk, G * 64))
        for t in range(chunk):
            y[t] = _step(c, s, xs[t])
        out.append(y.T.reshape(-1)[:n])
    return np.stack(out)


def loudness(x, fs: int, dtype=np.float64, y=None):
    """(L, threshold, gated blocks, l_j (J,)) of x, (n,) or (C, n) with C <= 2; dtype is the filter's arithmetic (float64: the
    definition; float32: the evaluation the bound is taken from); with y (C, n), the K-weighted channels are taken from there."""
    x = np.atleast_2d(np.asarray(x))
    assert x.shape[0] in (1, 2)
    n = x.shape[1]
    y = weighted(x, fs, dtype) if y is None else y
    assert y.shape == x.shape
    J = blocks(n, fs)
    z = np.zeros(J, np.float64)
    for ch in range(x.shape[0]):
        q = y[ch].astype(np.float64) ** 2
        for j in range(J):
            lo, hi = j * fs // 10, (j + 4) * fs // 10
            z[j] += q[lo:hi].sum() / (hi - lo)
    l = lufs(z)
    keep = l > -70.0
    if not keep.any():
        return -math.inf, -math.inf, 0, l
    gamma = float(lufs(z[keep].mean())) - 10.0
    keep &= l > gamma
    return float(lufs(z[keep].mean())), gamma, int(keep.sum()), l


def ulp32(v: float) -> float:
    return float(np.spacing(np.float32(abs(v))))


def bound(want64: float, got32: float) -> float:
    """What a value may differ from float64 by: the fp32 evaluation's own error, at least two fp32 ulps of the value."""
    if not math.isfinite(want64):
        return 0.0
    return max(abs(got32 - want64), 2.0 * ulp32(want64))


def bound64(want64: float, standin64: float) -> float:
    """What a value of a device that filters in fp64 may differ from float64 by: two fp32 ulps of the value (it is stored as fp32)
    plus four times what the chunked evaluation in float64 (weighted_chunked) differs from the sequential one by (four: the
    device's order of products and sums inside a step is not the stand-in's)."""
    if not math.isfinite(want64):
        return 0.0
    return 2.0 * ulp32(want64) + 4.0 * abs(standin64 - want64)


def gate_margin(x, fs: int) -> float:
    """The least distance of a block of x from either gate, in LU (inf without a finite block)."""
    L, gamma, _count, l = loudness(x, fs)
    l = l[np.isfinite(l)]
    if l.size == 0:
        return math.inf
    d = np.abs(l + 70.0).min()
    return float(min(d, np.abs(l - gamma).min())) if math.isfinite(gamma) else float(d)


def make_clip(n: int, seed: int, amplitude: float = 0.3) -> np.ndarray:
    """n fp32 samples: white noise of the given standard deviation with a slow envelope."""
    rng = np.random.default_rng(seed)
    env = 0.6 + 0.4 * np.sin(np.arange(n) * (2 * np.pi / 30011.0))
    return (rng.standard_normal(n) * env * amplitude).astype(np.float32)


def make_low_clip(n: int, fs: int, seed: int) -> np.ndarray:
    """A 30 Hz tone of 0.5 plus a DC offset of 0.3 plus noise of 0.01: nearly all of it under the high pass."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (0.5 * np.sin(2 * np.pi * 30.0 * t) + 0.3 + 0.01 * rng.standard_normal(n)).astype(np.float32)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.5


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def measure(clips, fs: int, momentary: bool = True):
    """One wt_loudness over clips (fp32 views on the GPU, (n,) or (C, n) with unit sample stride): returns ((B, 3) fp32 on the
    CPU, [l_j per clip on the CPU]); checks that nothing is written behind the workspace or the blocks."""
    from wavtokenizer_amd import _capi
    B = len(clips)
    out = torch.full((B, 3), SENTINEL, dtype=torch.float32, device="cuda")
    Js = [int(_capi.lib.wt_loudness_blocks(c.shape[-1], fs)) for c in clips]
    blk = [torch.full((J + 2,), SENTINEL, dtype=torch.float32, device="cuda") for J in Js]
    descs = (_capi.WtLoudnessClip * B)()
    total = 0
    for j, (d, c) in enumerate(zip(descs, clips)):
        assert c.dtype == torch.float32 and c.dim() in (1, 2) and c.stride(-1) == 1
        d.x, d.n, d.channels = c.data_ptr(), c.shape[-1], (1 if c.dim() == 1 else c.shape[0])
        d.channel_stride = c.stride(0) if c.dim() == 2 else 0
        d.out, d.blocks = out.data_ptr() + 12 * j, (blk[j].data_ptr() if momentary else None)
        total += d.n * d.channels
    nbytes = int(_capi.lib.wt_loudness_workspace_bytes(B, total))
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(_capi.lib.wt_loudness(descs, B, fs, ctypes.c_void_p(ws.data_ptr()), _stream()), "wt_loudness")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xAB).all()), "wt_loudness wrote behind its workspace"
    for J, b in zip(Js, blk):
        assert bool((b[J:] == SENTINEL).all()) and (momentary or bool((b == SENTINEL).all())), "wt_loudness wrote behind the blocks"
    return out.cpu().numpy(), [b[:J].cpu().numpy() for J, b in zip(Js, blk)]


def normalize_rows_lufs(rows, n, fs: int, target: float):
    """wt_normalize_rows_lufs in place on rows (B, T_pad) fp32 on the GPU; returns the scales (B,)."""
    from wavtokenizer_amd import _capi
    B, T_pad = rows.shape
    scales = torch.full((B,), -7.0, dtype=torch.float32, device="cuda")
    nbytes = int(_capi.lib.wt_normalize_rows_lufs_workspace_bytes(B, T_pad))
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(_capi.lib.wt_normalize_rows_lufs(ctypes.c_void_p(rows.data_ptr()), B, T_pad, (ctypes.c_int64 * B)(*n), fs, target,
                                                 ctypes.c_void_p(scales.data_ptr()), ctypes.c_void_p(ws.data_ptr()), _stream()),
                "wt_normalize_rows_lufs")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xAB).all()), "wt_normalize_rows_lufs wrote behind its workspace"
    return scales
