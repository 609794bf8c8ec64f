"""The host side of STOI (csrc/stoi.hip, wavtokenizer_amd/metrics.py) without a GPU: the exports, the tables a handle uploads
against the float64 definition (tests/stoi_ref.py), the closed-form resampler against scipy, the refusals, made with fake pointers
and a fake handle of a device no test machine has current, so that nothing can ever be launched, and the float64 definition
itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import stoi_ref as R
from wavtokenizer_amd import _capi, metrics
from wavtokenizer_amd._capi import WT_ERR_INVALID, WtStoiClip, WtStoiTaps, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOI_EXPORTS = {"wt_stoi_create", "wt_stoi_destroy", "wt_stoi_resampled_length", "wt_stoi_tables", "wt_stoi_workspace_bytes", "wt_stoi"}


class FakeStoi(ctypes.Structure):
    """struct wt_stoi_handle of csrc/stoi.hip."""
    _fields_ = [("device", ctypes.c_int), ("sample_rate", ctypes.c_int), ("p", ctypes.c_int), ("q", ctypes.c_int), ("L", ctypes.c_int),
                ("tab", ctypes.c_void_p)]


def fake_handle(fs=24000, device=63, **over):
    _h, p, q, L = R.resample_filter(fs)
    f = dict(device=device, sample_rate=fs, p=p, q=q, L=L, tab=0x7000000000)
    f.update(over)
    return FakeStoi(f["device"], f["sample_rate"], f["p"], f["q"], f["L"], f["tab"])


def _tables(fs):
    p, q, L = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.wt_stoi_tables(fs, ctypes.byref(p), ctypes.byref(q), ctypes.byref(L), None, None, None) == 0
    filt = np.zeros(2 * L.value + 1, np.float32)
    window = np.zeros(256, np.float32)
    edges = np.zeros(16, np.int32)
    assert lib.wt_stoi_tables(fs, None, None, None, filt.ctypes.data_as(ctypes.c_void_p), window.ctypes.data_as(ctypes.c_void_p),
                              edges.ctypes.data_as(ctypes.c_void_p)) == 0
    return p.value, q.value, L.value, filt, window, edges


def test_header_and_capi_agree_on_the_stoi_exports():
    header = open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")).read()
    declared = {s for s in re.findall(r"\b(wt_[a-z0-9_]+)\s*\(", header) if s.startswith("wt_stoi")}
    assert declared == STOI_EXPORTS
    assert STOI_EXPORTS <= set(_capi.EXPORTS)
    for sym in STOI_EXPORTS:
        assert getattr(lib, sym) is not None
    assert ctypes.sizeof(WtStoiClip) == 32 and ctypes.sizeof(WtStoiTaps) == 32


@pytest.mark.parametrize("fs", [24000, 16000, 44100, 8000])
def test_closed_form_resampler_is_scipy_resample_poly(fs):
    signal = pytest.importorskip("scipy.signal")
    p, q = R.ratio(fs)
    for T in (1, 700, 5001):
        x = np.random.default_rng(T).standard_normal(T)
        want = signal.resample_poly(x, p, q, window=R.octave_window(fs))
        got = R._resample(x, fs, np.float64)
        assert got.shape == want.shape == (R.resampled_length(T, fs),)
        assert float(np.abs(got - want).max()) <= 1e-12 * float(np.abs(want).max()), (fs, T)


@pytest.mark.parametrize("fs", R.RATES)
def test_tables_are_the_float64_definition_rounded_once(fs):
    p, q, L, filt, window, edges = _tables(fs)
    h64, p64, q64, L64 = R.resample_filter(fs)
    assert (p, q, L) == (p64, q64, L64) == (*R.ratio(fs), L64)
    h32 = h64.astype(np.float32)
    assert np.array_equal(filt, h32)
    assert abs(float(filt.astype(np.float64).sum()) - p) <= 1e-5 * p
    w32 = R.window64().astype(np.float32)
    assert np.array_equal(window, w32)
    assert window[0] > 0 and np.array_equal(window, window[::-1])
    assert [tuple(e) for e in zip(edges[:-1], edges[1:])] == list(R.BAND_EDGES) == list(R.band_edges())


def test_the_24_khz_filter_and_the_rates():
    p, q, L, filt, _w, _e = _tables(24000)
    assert (p, q, L) == (5, 12, 435) and filt.shape == (871,)
    for fs in (0, -5, 12345, 22051, 96001):
        assert lib.wt_stoi_tables(fs, None, None, None, None, None, None) == WT_ERR_INVALID, fs
        h = ctypes.c_void_p()
        assert lib.wt_stoi_create(fs, 0, ctypes.byref(h)) == WT_ERR_INVALID and not h.value and lib.wt_last_error()
        if fs > 0:
            with pytest.raises(ValueError):
                metrics.stoi_ratio(fs)
    assert lib.wt_stoi_create(24000, 0, None) == WT_ERR_INVALID
    for fs in R.RATES:
        assert metrics.stoi_ratio(fs) == R.ratio(fs)


def test_lengths_and_workspace():
    h = fake_handle(24000)
    for T, n in ((0, 0), (1, 1), (12, 5), (13, 6), (9830, 4096), (9831, 4097), (72000, 30000)):
        assert lib.wt_stoi_resampled_length(ctypes.byref(h), T) == n == R.resampled_length(T, 24000), T
    assert lib.wt_stoi_resampled_length(None, 100) == -1 and lib.wt_stoi_resampled_length(ctypes.byref(h), -1) == -1
    assert lib.wt_stoi_resampled_length(ctypes.byref(fake_handle(R.FS)), 4097) == 4097
    for n, k0 in ((256, 0), (257, 1), (384, 1), (385, 2), (4096, 30), (4097, 31), (4225, 32)):
        assert R.candidate_frames(n) == k0
    assert metrics.stoi_frames(9831, 24000) == (4097, 31) and metrics.stoi_frames(4225, 10000) == (4225, 32)
    with pytest.raises(ValueError, match="256"):
        metrics.stoi_frames(614, 24000)                             # 256 samples at 10 kHz
    assert metrics.stoi_frames(615, 24000) == (257, 1)
    assert lib.wt_stoi_workspace_bytes(ctypes.byref(h), 3, 100, 10) == 240 + 4 * (200 + 330 + 6)
    assert lib.wt_stoi_workspace_bytes(None, 3, 100, 10) == 0 and lib.wt_stoi_workspace_bytes(ctypes.byref(h), 0, 100, 10) == 0


A, B_, OUT, WS = 0x7100000000, 0x7200000000, 0x7300000000, 0x7400000000


def _clips(n=1, **over):
    descs = (WtStoiClip * n)()
    for i in range(n):
        descs[i].clean, descs[i].processed, descs[i].length, descs[i].out = A, B_, 12000, OUT
    for k, v in over.items():
        setattr(descs[n - 1], k, v)
    return descs


def _refused(call, what):
    assert call() == WT_ERR_INVALID, what
    msg = lib.wt_last_error().decode()
    assert msg.startswith("wt_stoi"), (what, msg)
    return msg


@pytest.mark.parametrize("extended", [0, 1])
def test_every_refusal_is_made_before_any_device_call(extended):
    h = fake_handle()
    ws = ctypes.c_void_p(WS)

    def call(handle=h, clips=None, n=1, workspace=ws, taps=None):
        hp = ctypes.byref(handle) if handle is not None else None
        clips = _clips(n) if clips is None else clips
        return lambda: lib.wt_stoi(hp, clips, n, extended, workspace, None, ctypes.byref(taps) if taps is not None else None)

    assert "null handle" in _refused(call(handle=None), "null handle")
    assert "null clean" in _refused(call(clips=_clips(clean=None)), "null clean")
    assert "null processed" in _refused(call(clips=_clips(processed=None)), "null processed")
    assert "null out" in _refused(call(clips=_clips(out=None)), "null out")
    assert "clip 2: null clean" in _refused(call(clips=_clips(3, clean=None), n=3), "the last of three")
    assert "256" in _refused(call(clips=_clips(length=614)), "256 samples at 10 kHz")
    assert "length" in _refused(call(clips=_clips(length=0)), "length 0")
    assert "length" in _refused(call(clips=_clips(length=-4)), "negative length")
    assert "256" in _refused(call(handle=fake_handle(R.FS), clips=_clips(length=256)), "256 samples, no resampling")
    assert "misaligned" in _refused(call(clips=_clips(clean=A + 2)), "misaligned clean")
    assert "misaligned" in _refused(call(clips=_clips(processed=B_ + 2)), "misaligned processed")
    assert "misaligned" in _refused(call(clips=_clips(out=OUT + 1)), "misaligned out")
    assert "misaligned tap" in _refused(call(taps=WtStoiTaps(A + 1, None, None, None)), "misaligned tap")
    assert "workspace" in _refused(call(workspace=ctypes.c_void_p(WS + 4)), "misaligned workspace")
    assert "workspace" in _refused(call(workspace=None), "null workspace")
    assert "B outside" in _refused(call(n=0), "B = 0")
    assert "B outside" in _refused(lambda: lib.wt_stoi(ctypes.byref(h), _clips(1), 32768, extended, ws, None, None), "B = 32768")
    # a sound call on a handle of device 63: refused for the device (no machine here has 64 GPUs and the last one current)
    assert "another device" in _refused(call(), "handle of another device")
    assert "another device" in _refused(call(clips=_clips(length=615)), "the shortest clip")
    assert "another device" in _refused(call(handle=fake_handle(R.FS), clips=_clips(length=257)), "the shortest clip at 10 kHz")
    assert "another device" in _refused(call(n=40, clips=_clips(40)), "handle of another device, workspace path")
    assert "another device" in _refused(call(taps=WtStoiTaps(A, B_, OUT, WS)), "with taps")
    for bad in (dict(p=6), dict(L=434), dict(tab=None), dict(sample_rate=0), dict(sample_rate=12345, p=2000, q=2469)):
        assert "handle" in _refused(call(handle=fake_handle(**bad)), bad)


def test_python_surface_refuses_bad_arguments_and_cpu_tensors():
    a, b = torch.zeros(12000), torch.zeros(12001)
    with pytest.raises(ValueError, match="lengths 12000 and 12001 differ"):
        metrics.stoi_many([a], [b])
    with pytest.raises(ValueError, match="as many"):
        metrics.stoi_many([a], [a, a])
    with pytest.raises(ValueError, match="one per pair"):
        metrics.stoi_many([a, a], [a, a], sample_rate=[24000])
    for rates in (np.array([24000]), torch.tensor([24000]), range(24000, 24001), np.array([24000, 16000, 8000])):
        with pytest.raises(ValueError, match="one per pair"):                  # any sequence of rates counts as one per pair
            metrics.stoi_many([a, a], [a, a], sample_rate=rates)
    for rates in (np.array([24000, 16000]), torch.tensor([24000, 16000]), np.int64(24000), np.array(24000)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            metrics.stoi_many([a, a], [a, a], sample_rate=rates)
    with pytest.raises(ValueError, match="beyond 441"):
        metrics.stoi_many([a, a], [a, a], sample_rate=np.array([24000, 12345]))
    with pytest.raises(ValueError, match="positive integer"):
        metrics.stoi_many([a], [a], sample_rate="24000")
    with pytest.raises(ValueError, match="shapes"):
        metrics.stoi(a, b)
    with pytest.raises(ValueError, match="must be"):
        metrics.stoi(torch.zeros(2, 2, 12000), torch.zeros(2, 2, 12000))
    with pytest.raises(ValueError, match="beyond 441"):
        metrics.stoi(a, a, 22051)
    with pytest.raises(ValueError, match="beyond 441"):
        metrics.stoi_many([a], [a], sample_rate=[12345])
    with pytest.raises(ValueError, match="256"):
        metrics.stoi(a[:614], a[:614])
    with pytest.raises(ValueError, match="256"):
        metrics.stoi_many([a, a[:600]], [a, a[:600]])
    for call in (lambda: metrics.stoi(a, a), lambda: metrics.stoi_many([a], [a]), lambda: metrics.stoi(torch.zeros(2, 1, 12000), torch.zeros(2, 1, 12000)),
                 lambda: metrics.stoi_many([a, a], [a, a], sample_rate=[24000, 16000], extended=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(ARCH_HOP600)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.round_trip_stoi([torch.zeros(12000)])


def test_the_float64_definition():
    fs = 10000
    x = R.speechlike(3 * fs, fs)
    for ext in (False, True):
        assert abs(R.stoi64(x, x, fs, ext) - 1.0) <= 1e-9
        d = [R.stoi64(x, R.noisy(x, snr), fs, ext) for snr in (20, 0, -10)]
        assert 1.0 > d[0] > d[1] > d[2] > 0.0, (ext, d)
    d = [R.stoi64(x, R.noisy(x, snr), fs) for snr in (20, 0, -10)]
    assert d[0] > 0.9 and 0.5 < d[1] < 0.9 and d[2] < 0.5, d
    # fewer than 30 frames: 4096 samples have K0 = 30 candidate frames, J = 29
    assert R.stoi64(x[:4096], x[:4096], fs) == R.SHORT == 1e-5 and R.stoi64(x[:4096], x[:4096], fs, True) == 1e-5
    assert abs(R.stoi64(x[:4097], x[:4097], fs) - 1.0) <= 1e-9
    # the fp32 stand-in follows the definition closely
    s = R.stages(x.astype(np.float64), R.noisy(x, 0).astype(np.float64), fs)
    s32 = R.stages(x, R.noisy(x, 0), fs, np.float32)
    assert np.array_equal(s.keep, s32.keep) and abs(float(s32.d[False]) - s.d[False]) < 1e-5


def test_the_cpu_side_of_the_rate_and_edge_tests():
    """What tests/test_stoi_rates.py and tests/test_stoi_edges.py assert before they launch: the (K0, K) expectations, the margin and
    condition numbers, the stand-in's sanity windows, and that the definition and the stand-in give exact zeros, leave the keep mask
    alone under the edge test's change of the clean signal and are invariant under a power-of-two gain."""
    from tests import test_stoi_edges, test_stoi_rates
    cases, bars = test_stoi_rates.reference()
    assert len(cases) == 3 * 5 + 2 and all(b > 0 for b in bars.values())
    cases, bars = test_stoi_edges.reference()
    assert all(b > 0 for b in bars.values())
    assert len(test_stoi_edges.zero_pairs()) == 3
    assert [int(c[2].sum()) for c in test_stoi_edges.eps_scale()] == [35, 45]
    assert len(test_stoi_edges.influence()[5]) == 2
    assert sorted(test_stoi_edges.gain_pairs()) == [10000, 24000]
