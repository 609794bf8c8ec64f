"""The host side of SI-SDR and SNR (csrc/wavedist.hip, wavtokenizer_amd/metrics.py) without a GPU: the exports, the workspace
size, every refusal, made with fake pointers so that nothing can ever be launched, the Python argument checks, and the two
CPU references of tests/wavedist_ref.py against each other and against the table of the definition."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import wavedist_ref as R
from wavtokenizer_amd import _capi, metrics
from wavtokenizer_amd._capi import WT_ERR_INVALID, WtWavedistClip, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVEDIST_EXPORTS = {"wt_wavedist_workspace_bytes", "wt_wavedist_block", "wt_wavedist"}


def test_header_capi_and_library_agree_on_the_wavedist_exports():
    header = open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")).read()
    declared = {s for s in re.findall(r"\b(wt_[a-z0-9_]+)\s*\(", header) if s.startswith("wt_wavedist")}
    assert declared == WAVEDIST_EXPORTS
    assert WAVEDIST_EXPORTS <= set(_capi.EXPORTS)
    for sym in WAVEDIST_EXPORTS:
        assert getattr(lib, sym) is not None
    assert ctypes.sizeof(WtWavedistClip) == 32


def test_block_and_workspace():
    blk = R.block()
    assert blk >= 256 and blk % 256 == 0
    # descriptors (40 bytes each, rounded up to 16) | 4 floats per pair | 3 floats per block, a pair of T samples has at most T / blk + 1
    assert lib.wt_wavedist_workspace_bytes(3, 10 * blk + 5) == 128 + 48 + 12 * (10 + 3)
    assert lib.wt_wavedist_workspace_bytes(1, 1) == 48 + 16 + 12
    assert lib.wt_wavedist_workspace_bytes(0, 10) == 0 and lib.wt_wavedist_workspace_bytes(1, -1) == 0


P, T_, OUT, WS = 0x7100000000, 0x7200000000, 0x7300000000, 0x7400000000


def _clips(n=1, **over):
    descs = (WtWavedistClip * n)()
    for i in range(n):
        descs[i].estimate, descs[i].target, descs[i].length, descs[i].out = P, T_, 3000, OUT
    for k, v in over.items():
        setattr(descs[n - 1], k, v)
    return descs


def _refused(call, what):
    assert call() == WT_ERR_INVALID, what
    msg = lib.wt_last_error().decode()
    assert msg.startswith("wt_wavedist"), (what, msg)
    return msg


@pytest.mark.parametrize("zero_mean", [0, 1])
def test_every_refusal_is_made_before_any_device_call(zero_mean):
    ws = ctypes.c_void_p(WS)

    def call(clips=None, n=1, workspace=ws):
        clips = _clips(n) if clips is None else clips
        return lambda: lib.wt_wavedist(clips, n, zero_mean, workspace, None)

    assert "null clips" in _refused(lambda: lib.wt_wavedist(None, 1, zero_mean, ws, None), "null clips")
    assert "workspace" in _refused(call(workspace=None), "null workspace")
    assert "workspace" in _refused(call(workspace=ctypes.c_void_p(WS + 4)), "misaligned workspace")
    assert "B outside" in _refused(call(n=0), "B = 0")
    assert "B outside" in _refused(call(n=65536, clips=_clips(1)), "B = 65536")
    assert "null estimate" in _refused(call(clips=_clips(estimate=None)), "null estimate")
    assert "null out" in _refused(call(clips=_clips(out=None)), "null out")
    assert "null target" in _refused(call(clips=_clips(target=None)), "null target")
    assert "clip 2: null target" in _refused(call(clips=_clips(3, target=None), n=3), "the last of three")
    assert "length" in _refused(call(clips=_clips(length=0)), "length 0")
    assert "length" in _refused(call(clips=_clips(length=-5)), "length -5")
    assert "misaligned" in _refused(call(clips=_clips(estimate=P + 2)), "misaligned estimate")
    assert "misaligned" in _refused(call(clips=_clips(target=T_ + 1)), "misaligned target")
    assert "misaligned" in _refused(call(clips=_clips(out=OUT + 2)), "misaligned out")
    # the order is mel_run's: the call's own arguments, then the clips in order
    assert "workspace" in _refused(call(workspace=None, n=0), "clips and workspace before B")
    assert "B outside" in _refused(call(n=0, clips=_clips(estimate=None)), "B before the clips")
    assert "null estimate" in _refused(call(clips=_clips(estimate=None, length=0)), "a clip's pointers before its length")
    assert "length" in _refused(call(clips=_clips(length=0, out=OUT + 1)), "its length before its alignment")


def test_python_surface_checks_its_arguments():
    a, b = torch.zeros(3000), torch.zeros(3001)
    for many, one in ((metrics.si_sdr_many, metrics.si_sdr), (metrics.snr_many, metrics.snr)):
        with pytest.raises(ValueError, match="lengths 3000 and 3001 differ"):
            many([a], [b])
        with pytest.raises(ValueError, match="as many"):
            many([a], [a, a])
        with pytest.raises(ValueError, match="shapes"):
            one(a, b)
        with pytest.raises(ValueError, match="empty"):
            one(a[:0], a[:0])
        with pytest.raises(ValueError, match="1-D"):
            many([torch.zeros(2, 30)], [torch.zeros(2, 30)])
        with pytest.raises(ValueError, match=r"\(T,\), \(B, T\) or \(B, 1, T\)"):
            one(torch.zeros(2, 2, 30), torch.zeros(2, 2, 30))
        for call in (lambda: many([a], [a]), lambda: one(a, a), lambda: one(a, a, zero_mean=True),
                     lambda: one(torch.zeros(2, 1, 30), torch.zeros(2, 1, 30))):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()


def test_the_references_agree_and_the_moment_form_does_not():
    """The fp32 stand-in (three passes, residuals sample by sample) stays within 1e-3 dB of float64 up to 100 dB; the expanded-moment
    form in fp32 is off by more than 1 dB at 94 dB (the definition's table): the reason the kernels may not use it."""
    for sdr in (10.0, 40.0, 70.0, 94.0, 100.0):
        p, t = R.pair(72000, sdr)
        want = R.measures64(p, t)
        got = R.standin_fp32(p, t)
        s = 0.64 * float((t.astype(np.float64) ** 2).sum())                    # (eps = 2^-23 in the denominator shows above 80 dB)
        made = 10 * np.log10((s + R.EPS) / (s * 10 ** (-sdr / 10) + R.EPS))
        assert abs(want[0] - made) < 0.05 and abs(got[0] - want[0]) < 1e-3 and abs(got[1] - want[1]) < 1e-3, (sdr, made, want, got)
    p, t = R.pair(72000, 94.0)
    f32 = np.float32
    spp, spt, stt = (p * p).sum(dtype=f32), (p * t).sum(dtype=f32), (t * t).sum(dtype=f32)
    alpha = f32(spt / stt)
    moment = 10 * np.log10(float(f32(alpha * alpha * stt)) / float(f32(f32(alpha * alpha * stt) - f32(2) * f32(alpha * spt) + spp)))
    assert not abs(moment - R.measures64(p, t)[0]) < 1.0
    # zero_mean takes a DC offset out; silence gives exactly 0 dB
    p, t = R.pair(5000, 40.0, dc=0.5, level=0.01)
    assert abs(R.measures64(p, t, zero_mean=True)[0] - 40.0) < 0.05 and R.measures64(p, t)[0] > 45.0
    z = np.zeros(100, np.float32)
    assert R.measures64(z, z) == (0.0, 0.0) and R.standin_fp32(z, z) == (0.0, 0.0)
