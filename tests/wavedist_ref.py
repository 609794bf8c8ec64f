"""SI-SDR and SNR of csrc/wavedist.hip (include/wavtokenizer_amd.h gives the definition) in float64 numpy, the fp32 stand-in that
serves as the yardstick for the kernels' rounding error (the three-pass direct form in fp32 on the CPU), and the pairs and ctypes
plumbing the tests share.  torchmetrics is not available here, so the parity with it is unpinned."""
import numpy as np

from tests.mel_ref import Arena, Outputs

EPS = 2.0 ** -23


def measures64(p, t, zero_mean=False):
    """(SI-SDR, SNR) in dB of estimate p against target t, in float64."""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    if zero_mean:
        p, t = p - p.mean(), t - t.mean()
    alpha = ((p * t).sum() + EPS) / ((t * t).sum() + EPS)
    si_sdr = 10.0 * np.log10((((alpha * t) ** 2).sum() + EPS) / (((alpha * t - p) ** 2).sum() + EPS))
    snr = 10.0 * np.log10(((t * t).sum() + EPS) / (((t - p) ** 2).sum() + EPS))
    return float(si_sdr), float(snr)


def standin_fp32(p, t, zero_mean=False):
    """The same three passes in float32 throughout: the means, then alpha from sum p t and sum t^2, then the residual energies
    sample by sample; every product and sum rounded to float32 (numpy's pairwise sums)."""
    f32 = np.float32
    p, t = np.asarray(p, f32), np.asarray(t, f32)
    if zero_mean:
        p = (p - f32(p.sum(dtype=f32) / f32(len(p)))).astype(f32)
        t = (t - f32(t.sum(dtype=f32) / f32(len(t)))).astype(f32)
    eps = f32(EPS)
    stt = (t * t).sum(dtype=f32)
    alpha = f32(((p * t).sum(dtype=f32) + eps) / (stt + eps))
    at = (alpha * t).astype(f32)
    res = ((at - p) ** 2).sum(dtype=f32)
    tgt = (at * at).sum(dtype=f32)
    noise = ((t - p) ** 2).sum(dtype=f32)
    si_sdr = f32(10) * np.log10(f32((tgt + eps) / (res + eps)), dtype=f32)
    snr = f32(10) * np.log10(f32((stt + eps) / (noise + eps)), dtype=f32)
    return float(si_sdr), float(snr)


def pair(T: int, sdr_db: float, seed: int = 0, level: float = 0.1, dc: float = 0.0):
    """(estimate, target) fp32: target = dc + level * white noise; estimate = dc + 0.8 (target - dc) + noise orthogonalised against
    the target and scaled so that the SI-SDR of the centred pair is sdr_db in float64 (before the rounding to fp32)."""
    rng = np.random.default_rng(1000 * seed + T)
    t = level * rng.standard_normal(T)
    n = rng.standard_normal(T)
    if T > 1:
        n = n - t * (n @ t) / (t @ t)
        n *= np.sqrt((0.8 * t) @ (0.8 * t) / (n @ n)) * 10.0 ** (-sdr_db / 20.0)
    else:
        n = np.zeros(T)
    return (dc + 0.8 * t + n).astype(np.float32), (dc + t).astype(np.float32)


def block() -> int:
    from wavtokenizer_amd._capi import lib
    return int(lib.wt_wavedist_block())


def run(estimates, targets, zero_mean=False, ws_fill=0xAB):
    """One wt_wavedist call on pairs laid out in a NaN arena, outputs between canaries, the workspace filled with ws_fill
    beforehand.  ([2] float32 arrays (SI-SDR, SNR), canaries intact)."""
    import ctypes

    import torch

    from wavtokenizer_amd._capi import WtWavedistClip, check, lib
    n = len(estimates)
    arena = Arena(list(estimates) + list(targets))
    outs = Outputs([2] * n)
    nbytes = int(lib.wt_wavedist_workspace_bytes(n, sum(len(c) for c in estimates)))
    ws = torch.full((nbytes + 64,), ws_fill, dtype=torch.uint8, device="cuda")
    descs = (WtWavedistClip * n)()
    for i in range(n):
        descs[i].estimate, descs[i].target, descs[i].length, descs[i].out = arena.ptr(i), arena.ptr(n + i), len(estimates[i]), outs.ptr(i)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.wt_wavedist(descs, n, 1 if zero_mean else 0, ctypes.c_void_p(ws.data_ptr()), stream), "wt_wavedist")
    torch.cuda.synchronize()
    got, intact = outs.read()
    assert bool((ws[nbytes:] == ws_fill).all()), "the call wrote behind its workspace"
    return got, intact
