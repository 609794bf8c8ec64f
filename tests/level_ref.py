"""Definitions, bounds and C-ABI wrappers for the level kernels (csrc/level.hip: wt_level, wt_normalize_rows, wt_scale_rows) and
the rescaling emit (csrc/audio.hip: wt_emit_rescaled): tests/test_level_op.py, test_emit_rescaled_op.py, test_level_calls.py and
test_level_host.py share them.

The definitions are the reference's three expressions on one mono clip, in torch fp32 on the CPU (what the kernels must equal bit
for bit where the arithmetic is order-free) and in float64 (what the one sum that has an order, the mean square, is measured
against):
    peak normalisation   extract_features.py:27-28     wav / (wav.abs().max() + 1e-8)
    rms scale            encoder/model.py:153-156      scale = 1e-8 + mono.pow(2).mean().sqrt();  x / scale
    rescale              encoder/utils.py:95-103       wav * min(limit / wav.abs().max(), 1)

The bound on the rms: the kernel squares n samples (one rounding each, relative 2^-24 = u), adds them in a binary tree whose depth
over non-zero leaves is at most D = ceil(log2 n) (every partial sum rounds once, all terms are non-negative: the sum errs by at
most (1 + u)^(D + 1) - 1 relative), divides by n once (u), takes the square root (which halves the relative error carried in
and rounds once more, u): (D + 2) u / 2 + u to first order, below (3 + ceil(log2 n)) u, the bound the tests assert."""
import ctypes
import math

import numpy as np
import torch

U = 2.0 ** -24


def rms_bound(n: int) -> float:
    """Relative error allowed on the rms of n samples (see above)."""
    return (3 + math.ceil(math.log2(n))) * U


def peak64(x) -> float:
    return float(np.abs(np.asarray(x, np.float64)).max())


def rms64(x) -> float:
    x = np.asarray(x, np.float64)
    return float(np.sqrt((x * x).sum() / x.shape[0]))


def peak_normalize(x: torch.Tensor, gain=None):
    """(y, scale) of a 1-D fp32 CPU clip: scale = max |x| + 1e-8, y = x / scale, times gain (an fp32 value) when given."""
    scale = x.abs().max() + 1e-8
    y = x / scale
    return (y if gain is None else y * torch.tensor(gain, dtype=torch.float32)), scale


def rms_normalize(x: torch.Tensor):
    """(y, scale) of a 1-D fp32 CPU clip: scale = 1e-8 + sqrt(mean x^2) with torch's own fp32 mean (its order is torch's: compare
    the scale within rms_bound, not bit for bit)."""
    scale = 1e-8 + x.pow(2).mean().sqrt()
    return x / scale, scale


def rescale_factor(x: torch.Tensor, limit: float) -> torch.Tensor:
    """min(limit / max |x|, 1) as an fp32 0-d tensor; 1 for a silent clip (0.99 / 0 = inf there: the same 1)."""
    mx = x.abs().max()
    return torch.minimum(torch.tensor(limit, dtype=torch.float32, device=x.device) / mx, torch.ones((), dtype=torch.float32, device=x.device)) \
        if float(mx) > 0 else torch.ones((), dtype=torch.float32, device=x.device)


def gain_of(target_db: float) -> float:
    """10^(target_db / 20) rounded to fp32."""
    return float(np.float32(10.0 ** (target_db / 20.0)))


def make_clip(n: int, seed: int, amplitude: float = 0.3) -> np.ndarray:
    """n fp32 samples: white noise of the given standard deviation with a slow envelope (a level that is not flat over the chunks)."""
    rng = np.random.default_rng(seed)
    env = 0.6 + 0.4 * np.sin(np.arange(n) * (2 * np.pi / 3001.0))
    return (rng.standard_normal(n) * env * amplitude).astype(np.float32)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def level(clips, out=None, total=None):
    """One wt_level over clips (1-D fp32 views on the GPU): returns (B, 2) fp32 = (peak, rms) per clip (or fills `out`)."""
    from wavtokenizer_amd import _capi
    B = len(clips)
    out = torch.full((B, 2), -7.0, dtype=torch.float32, device="cuda") if out is None else out
    descs = (_capi.WtLevelClip * B)()
    for j, (d, c) in enumerate(zip(descs, clips)):
        assert c.dtype == torch.float32 and c.dim() == 1 and c.stride(0) == 1
        d.x, d.n, d.out = c.data_ptr(), c.shape[0], out.data_ptr() + 8 * j
    nbytes = int(_capi.lib.wt_level_workspace_bytes(B, sum(c.shape[0] for c in clips) if total is None else total))
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(_capi.lib.wt_level(descs, B, ctypes.c_void_p(ws.data_ptr()), _stream()), "wt_level")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xAB).all()), "wt_level wrote behind its workspace"
    return out


def normalize_rows(rows, n, mode, gain=1.0):
    """wt_normalize_rows in place on rows (B, T_pad) fp32 on the GPU; returns the scales (B,)."""
    from wavtokenizer_amd import _capi
    B, T_pad = rows.shape
    scales = torch.full((B,), -7.0, dtype=torch.float32, device="cuda")
    nbytes = int(_capi.lib.wt_normalize_rows_workspace_bytes(B, T_pad))
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(_capi.lib.wt_normalize_rows(ctypes.c_void_p(rows.data_ptr()), B, T_pad, (ctypes.c_int64 * B)(*n), mode, gain,
                                            ctypes.c_void_p(scales.data_ptr()), ctypes.c_void_p(ws.data_ptr()), _stream()),
                "wt_normalize_rows")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xAB).all()), "wt_normalize_rows wrote behind its workspace"
    return scales


def scale_rows(rows, lens, scales):
    """wt_scale_rows in place: rows a list of 1-D fp32 views on the GPU, lens their valid lengths, scales (F,) fp32 on the GPU."""
    from wavtokenizer_amd import _capi
    table = torch.tensor([r.data_ptr() for r in rows], dtype=torch.int64).cuda()
    lengths = torch.tensor(list(lens), dtype=torch.int64).cuda()
    _capi.check(_capi.lib.wt_scale_rows(ctypes.c_void_p(table.data_ptr()), ctypes.c_void_p(lengths.data_ptr()),
                                        ctypes.c_void_p(scales.data_ptr()), len(rows), max(lens), _stream()), "wt_scale_rows")
    torch.cuda.synchronize()


def emit_rescaled(rows, n_in, rates, dests, limits):
    """One wt_emit_rescaled launch pair, the arguments of tests/emit_ref.py emit."""
    from tests import emit_ref as R
    from wavtokenizer_amd import _capi, audio
    dev = torch.cuda.current_device()
    B = len(rows)
    descs = (_capi.WtEmitClip * B)()
    for d, row, n, rate, dst, lim in zip(descs, rows, n_in, rates, dests, limits):
        d.src, d.n_in, d.resampler = row.data_ptr(), n, audio.resampler(R.CODEC_RATE, rate, dev)
        d.n_out = R.out_length(rate, n)
        assert d.n_out == dst.n_out
        d.dst = dst.buf.data_ptr() + dst.off * dst.buf.element_size()
        d.dtype = _capi.WT_EMIT_I16 if dst.buf.dtype == torch.int16 else _capi.WT_EMIT_F32
        d.channels, d.ch_stride, d.sample_stride, d.limit = dst.channels, dst.cs, dst.ss, lim
    nbytes = int(_capi.lib.wt_emit_rescaled_workspace_bytes(B))
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(_capi.lib.wt_emit_rescaled(descs, B, ctypes.c_void_p(ws.data_ptr()), _stream()), "wt_emit_rescaled")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xAB).all()), "wt_emit_rescaled wrote behind its workspace"
    return ws[:nbytes]
