"""The host side of the multi-resolution STFT distance (csrc/stftd.hip, wavtokenizer_amd/metrics.py) without a GPU: the exports,
the window a handle uploads against the float64 definition (tests/stftd_ref.py), the frame counts, and every refusal, made with
fake pointers and a fake handle of a device no test machine has current, so that nothing can ever be launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import stftd_ref as R
from wavtokenizer_amd import _capi, metrics
from wavtokenizer_amd._capi import WT_ERR_INVALID, WtStftdClip, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STFTD_EXPORTS = {"wt_stftd_create", "wt_stftd_destroy", "wt_stftd_frames", "wt_stftd_tables", "wt_stftd_workspace_bytes",
                 "wt_stftd_distance", "wt_stftd_magnitude"}


class FakeStftd(ctypes.Structure):
    """struct wt_stftd of csrc/stftd.hip."""
    _fields_ = [("device", ctypes.c_int), ("n_res", ctypes.c_int), ("n_fft", ctypes.c_int * 8), ("hop", ctypes.c_int * 8),
                ("win", ctypes.c_int * 8), ("off", ctypes.c_int * 8), ("tab", ctypes.c_void_p)]


def fake_handle(resolutions=R.RESOLUTIONS, device=63):
    h = FakeStftd()
    h.device, h.n_res, h.tab = device, len(resolutions), 0x7000000000
    off = 0
    for r, (n_fft, hop, win) in enumerate(resolutions):
        h.n_fft[r], h.hop[r], h.win[r], h.off[r] = n_fft, hop, win, off
        off += 3 * n_fft
    return h


def _int32s(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_header_capi_and_library_agree_on_the_stftd_exports():
    header = open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")).read()
    declared = {s for s in re.findall(r"\b(wt_[a-z0-9_]+)\s*\(", header) if s.startswith("wt_stftd")}
    assert declared == STFTD_EXPORTS
    assert STFTD_EXPORTS <= set(_capi.EXPORTS)
    for sym in STFTD_EXPORTS:
        assert getattr(lib, sym) is not None
    assert ctypes.sizeof(WtStftdClip) == 32


@pytest.mark.parametrize("n_fft,win", [(1024, 600), (2048, 1200), (512, 240), (1024, 599), (512, 512)])
def test_window_is_the_float64_definition_rounded_once(n_fft, win):
    window = np.full(n_fft, np.nan, np.float32)
    assert lib.wt_stftd_tables(n_fft, win, window.ctypes.data_as(ctypes.c_void_p)) == 0
    w64 = R.window64(n_fft, win)
    w32 = w64.astype(np.float32)
    assert bool((np.abs(window.astype(np.float64) - w32) <= np.spacing(w32)).all())
    left = (n_fft - win) // 2
    assert bool((window[:left + 1] == 0).all()) and bool((window[left + win:] == 0).all())      # (the window's own first sample is 0)
    assert bool((window[left + 1:left + win] > 0).all())
    if win % 2 == 0:
        assert window[left + win // 2] == 1
    import torch
    padded = torch.zeros(n_fft, dtype=torch.float64)
    padded[left:left + win] = torch.hann_window(win, periodic=True, dtype=torch.float64)
    assert float(np.abs(padded.numpy() - w64).max()) < 1e-15


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_window_is_torch_hann_window_at_the_edges_of_win_length(n_fft):
    """torch.hann_window(win_length, periodic=True) centred in n_fft and rounded once, down to one sample: torch gives [1.] there,
    where 0.5 - 0.5 cos 0 alone would give an all-zero window, every magnitude the floor and every distance 0."""
    for win in (1, 2, 3, n_fft - 1, n_fft):
        window = np.full(n_fft, np.nan, np.float32)
        assert lib.wt_stftd_tables(n_fft, win, window.ctypes.data_as(ctypes.c_void_p)) == 0
        left = (n_fft - win) // 2
        padded = torch.zeros(n_fft, dtype=torch.float64)
        padded[left:left + win] = torch.hann_window(win, periodic=True, dtype=torch.float64)
        want = padded.numpy().astype(np.float32)
        # (two float64 cosines may differ in their last bit, which can move the one rounding to fp32 by an ulp at a near-tie)
        assert bool((np.abs(window.astype(np.float64) - want) <= np.spacing(want)).all()), (n_fft, win)
        assert np.array_equal(window == 0, want == 0), (n_fft, win)
        if win <= 3:
            assert np.array_equal(window, want), (n_fft, win, window[left:left + win])
            assert np.array_equal(window[left:left + win], {1: [1.0], 2: [0.0, 1.0], 3: [0.0, 0.75, 0.75]}[win])
        assert float(np.abs(padded.numpy() - R.window64(n_fft, win)).max()) < 1e-15, (n_fft, win)
    assert left == 0 and window[0] == 0 and bool((window[1:] > 0).all())


def test_tables_and_create_refuse_other_parameters_before_any_device_call():
    for n_fft, win in ((256, 100), (4096, 100), (1000, 100), (1024, 0), (1024, 1025)):
        assert lib.wt_stftd_tables(n_fft, win, None) == WT_ERR_INVALID, (n_fft, win)
    assert lib.wt_stftd_tables(1024, 600, None) == 0
    bad = [((256,), (64,), (256,)), ((1024,), (0,), (600,)), ((1024,), (1025,), (600,)), ((1024,), (120,), (0,)), ((1024,), (120,), (1025,)),
           ((1024, 1000), (120, 120), (600, 600)), ((), (), ()), ((512,) * 9, (50,) * 9, (240,) * 9)]
    for n_fft, hop, win in bad:
        h = ctypes.c_void_p()
        rc = lib.wt_stftd_create(len(n_fft), _int32s(n_fft), _int32s(hop), _int32s(win), 0, ctypes.byref(h))
        assert rc == WT_ERR_INVALID and not h.value and lib.wt_last_error().decode().startswith("wt_stftd_create"), (n_fft, hop, win)
    assert lib.wt_stftd_create(1, _int32s((1024,)), _int32s((120,)), _int32s((600,)), 0, None) == WT_ERR_INVALID
    h = ctypes.c_void_p()
    assert lib.wt_stftd_create(1, None, _int32s((120,)), _int32s((600,)), 0, ctypes.byref(h)) == WT_ERR_INVALID


def test_frames_and_workspace():
    h = fake_handle()
    want = {(0, 512): -1, (0, 513): 5, (0, 599): 5, (0, 600): 6, (0, 72000): 601, (1, 1024): -1, (1, 1025): 5, (1, 72000): 301,
            (2, 256): -1, (2, 257): 6, (2, 72000): 1441, (3, 72000): -1, (-1, 72000): -1}
    for (r, T), f in want.items():
        assert lib.wt_stftd_frames(ctypes.byref(h), r, T) == f, (r, T)
        if f > 0:
            n_fft, hop, _win = R.RESOLUTIONS[r]
            assert metrics.stft_frames(T, n_fft, hop) == f == R.n_frames(T, hop)
    with pytest.raises(ValueError):
        metrics.stft_frames(1024, 2048, 240)
    assert lib.wt_stftd_frames(None, 0, 4096) == -1
    assert lib.wt_stftd_workspace_bytes(ctypes.byref(h), 3, 10) == 128 + 120        # 3 descriptors of 40 bytes rounded up to 16, 3 floats per frame
    assert lib.wt_stftd_workspace_bytes(ctypes.byref(h), 0, 10) == 0 and lib.wt_stftd_workspace_bytes(None, 3, 10) == 0


X, Y, OUT, WS = 0x7100000000, 0x7200000000, 0x7300000000, 0x7400000000


def _clips(n=1, **over):
    descs = (WtStftdClip * n)()
    for i in range(n):
        descs[i].estimate, descs[i].target, descs[i].length, descs[i].out = X, Y, 3000, OUT
    for k, v in over.items():
        setattr(descs[n - 1], k, v)
    return descs


def _refused(call, what):
    assert call() == WT_ERR_INVALID, what
    msg = lib.wt_last_error().decode()
    assert msg.startswith("wt_stftd_"), (what, msg)
    return msg


@pytest.mark.parametrize("distance", [False, True])
def test_every_refusal_is_made_before_any_device_call(distance):
    h = fake_handle()
    ws = ctypes.c_void_p(WS)

    def call(handle=h, clips=None, n=1, workspace=ws, r=0):
        hp = ctypes.byref(handle) if handle is not None else None
        clips = _clips(n) if clips is None else clips
        if distance:
            return lambda: lib.wt_stftd_distance(hp, clips, n, workspace, None)
        return lambda: lib.wt_stftd_magnitude(hp, r, clips, n, workspace, None)

    assert "null handle" in _refused(call(handle=None), "null handle")
    assert "null estimate" in _refused(call(clips=_clips(estimate=None)), "null estimate")
    assert "null out" in _refused(call(clips=_clips(out=None)), "null out")
    assert "clip 2: null estimate" in _refused(call(clips=_clips(3, estimate=None), n=3), "the last of three")
    assert "length" in _refused(call(clips=_clips(length=1024 if distance else 512)), "length at n_fft / 2")
    assert "length" in _refused(call(clips=_clips(length=0)), "length 0")
    assert "misaligned" in _refused(call(clips=_clips(estimate=X + 2)), "misaligned estimate")
    assert "misaligned" in _refused(call(clips=_clips(out=OUT + 1)), "misaligned out")
    assert "workspace" in _refused(call(workspace=ctypes.c_void_p(WS + 4)), "misaligned workspace")
    assert "workspace" in _refused(call(workspace=None), "null workspace")
    assert "B outside" in _refused(call(n=0), "B = 0")
    assert "B outside" in _refused(call(n=65536, clips=_clips(1)), "B = 65536")
    if distance:
        assert "null target" in _refused(call(clips=_clips(target=None)), "null target")
        assert "misaligned" in _refused(call(clips=_clips(target=Y + 2)), "misaligned target")
    else:
        assert "another device" in _refused(call(clips=_clips(target=None)), "target ignored")
        assert "another device" in _refused(call(clips=_clips(length=513)), "resolution 0 alone needs 513")
        assert "length" in _refused(call(clips=_clips(length=1024), r=1), "resolution 1 needs 1025")
        assert "no such resolution" in _refused(call(r=3), "r = 3")
        assert "no such resolution" in _refused(call(r=-1), "r = -1")
    # the order is mel_run's: the call's own arguments, then the clips in order, then the device
    assert "null handle" in _refused(call(handle=None, workspace=None, n=0), "handle first")
    assert "workspace" in _refused(call(workspace=None, n=0), "then clips and workspace")
    assert "B outside" in _refused(call(n=0, clips=_clips(estimate=None)), "then B")
    assert "null estimate" in _refused(call(clips=_clips(estimate=None, length=0)), "a clip's pointers before its length")
    assert "length" in _refused(call(clips=_clips(length=0, out=OUT + 1)), "its length before its alignment")
    # a sound call on a handle of device 63: refused for the device (no machine here has 64 GPUs and the last one current)
    assert "another device" in _refused(call(), "handle of another device")
    assert "another device" in _refused(call(n=70, clips=_clips(70)), "handle of another device, workspace path")
    assert "handle" in _refused(call(handle=fake_handle(((1024, 0, 600),))), "not a handle")
    assert "handle" in _refused(call(handle=fake_handle(((1000, 100, 600),))), "not a handle")


def test_python_surface_checks_its_arguments():
    a, b = torch.zeros(3000), torch.zeros(3001)
    with pytest.raises(ValueError, match="lengths 3000 and 3001 differ"):
        metrics.stft_distance_many([a], [b])
    with pytest.raises(ValueError, match="as many"):
        metrics.stft_distance_many([a], [a, a])
    with pytest.raises(ValueError, match="shapes"):
        metrics.stft_distance(a, b)
    with pytest.raises(ValueError, match="too short"):
        metrics.stft_distance_many([a[:1024]], [a[:1024]])
    with pytest.raises(ValueError, match="too short"):
        metrics.stft_magnitude(a[:512])
    with pytest.raises(ValueError, match="512, 1024 or 2048"):
        metrics.stft_distance_many([a], [a], fft_sizes=(256,), hop_sizes=(64,), win_lengths=(256,))
    with pytest.raises(ValueError, match="1..n_fft"):
        metrics.stft_magnitude(a, 1024, 0, 600)
    with pytest.raises(ValueError, match="1..n_fft"):
        metrics.stft_magnitude(a, 1024, 120, 1025)
    with pytest.raises(ValueError, match="one length"):
        metrics.stft_distance_many([a], [a], fft_sizes=(512, 1024), hop_sizes=(50,), win_lengths=(240,))
    with pytest.raises(ValueError, match="1-D"):
        metrics.stft_distance_many([torch.zeros(2, 3000)], [torch.zeros(2, 3000)])
    with pytest.raises(ValueError, match=r"\(T,\), \(B, T\) or \(B, 1, T\)"):
        metrics.stft_distance(torch.zeros(2, 2, 3000), torch.zeros(2, 2, 3000))
    assert metrics.stft_resolutions() == R.RESOLUTIONS
    for call in (lambda: metrics.stft_distance_many([a], [a]), lambda: metrics.stft_distance(a, a), lambda: metrics.stft_magnitude(a),
                 lambda: metrics.stft_magnitude_many([a]), lambda: metrics.stft_distance(torch.zeros(2, 1, 3000), torch.zeros(2, 1, 3000))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(ARCH_HOP600)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.round_trip_report([torch.zeros(12000)])
