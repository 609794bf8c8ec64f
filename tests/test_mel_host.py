"""The host side of the mel metric (csrc/mel.hip, wavtokenizer_amd/metrics.py) without a GPU: the exports, the tables a handle
uploads against the float64 definition (tests/mel_ref.py), the frame count, and every refusal, made with fake pointers and a fake
handle of a device no test machine has current, so that nothing can ever be launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import mel_ref as R
from wavtokenizer_amd import _capi, metrics
from wavtokenizer_amd._capi import WT_ERR_INVALID, WtMelClip, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEL_EXPORTS = {"wt_mel_create", "wt_mel_destroy", "wt_mel_frames", "wt_mel_tables", "wt_mel_workspace_bytes", "wt_mel_spectrogram",
               "wt_mel_distance"}


class FakeMel(ctypes.Structure):
    """struct wt_mel of csrc/mel.hip."""
    _fields_ = [("device", ctypes.c_int), ("sample_rate", ctypes.c_int), ("n_fft", ctypes.c_int), ("hop", ctypes.c_int),
                ("n_mels", ctypes.c_int), ("tab", ctypes.c_void_p)]


def fake_handle(hop=256, n_mels=100, device=63):
    return FakeMel(device, 24000, 1024, hop, n_mels, 0x7000000000)


def test_header_and_capi_agree_on_the_mel_exports():
    header = open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")).read()
    declared = {s for s in re.findall(r"\b(wt_[a-z0-9_]+)\s*\(", header) if s.startswith("wt_mel")}
    assert declared == MEL_EXPORTS
    assert MEL_EXPORTS <= set(_capi.EXPORTS)
    for sym in MEL_EXPORTS:
        assert getattr(lib, sym) is not None
    assert ctypes.sizeof(WtMelClip) == 32


GRID = [(sr, m) for sr in (8000, 16000, 22050, 24000, 44100, 48000) for m in (1, 2, 63, 64, 65, 100, 127, 128)]   # tests/test_mel_params.py
ONE_EMPTY = {(44100, 127), (44100, 128), (48000, 127), (48000, 128)}      # a narrow low filter whose two edges fall between two bins


@pytest.mark.parametrize("sample_rate,n_mels", [(24000, 100), (16000, 100), (16000, 64)] + [p for p in GRID if p not in ((24000, 100), (16000, 100), (16000, 64))])
def test_tables_are_the_float64_definition_rounded_once(sample_rate, n_mels):
    window = np.zeros(1024, np.float32)
    fb = np.zeros((513, n_mels), np.float32)
    rc = lib.wt_mel_tables(sample_rate, 1024, n_mels, window.ctypes.data_as(ctypes.c_void_p), fb.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    w64, fb64 = R.tables(sample_rate, n_mels)
    w32 = w64.astype(np.float32)
    assert bool((np.abs(window.astype(np.float64) - w32) <= np.spacing(w32)).all())
    assert window[0] == 0 and window[512] == 1
    assert np.array_equal(fb == 0, fb64 == 0)
    nz = fb64 != 0
    rel = np.abs(fb.astype(np.float64)[nz] - fb64[nz]) / fb64[nz]
    assert float(rel.max()) <= 2.0 ** -23
    per_filter = (fb != 0).sum(axis=0)
    assert int((per_filter == 0).sum()) == (1 if (sample_rate, n_mels) in ONE_EMPTY else 0)      # no empty filter but at those four
    assert np.array_equal(np.nonzero(per_filter == 0)[0], R.empty_filters(sample_rate, n_mels))
    assert int((fb != 0).sum(axis=1).max()) <= 2                    # a bin feeds at most two filters
    # what the sparse form a handle uploads relies on (wt_mel_create): every filter's non-zero bins are one run, and the runs fit
    # the weight table
    for m in np.nonzero(per_filter)[0]:
        k = np.nonzero(fb[:, m])[0]
        assert k[-1] - k[0] + 1 == len(k), (m, k)
    assert int(per_filter.sum()) <= 2 * 513 + 6
    if n_mels >= 127 and sample_rate in (8000, 16000):
        assert int(per_filter.sum()) == 1013                        # (the fullest of the grid: every bin but the two outermost, nearly twice)
    if (sample_rate, n_mels) == (24000, 100):
        assert int((fb != 0).sum(axis=0).max()) <= 31


def test_tables_refuse_other_parameters():
    for sr, n_fft, n_mels in ((24000, 512, 100), (24000, 2048, 100), (24000, 1024, 0), (24000, 1024, 129), (1, 1024, 100)):
        assert lib.wt_mel_tables(sr, n_fft, n_mels, None, None) == WT_ERR_INVALID, (sr, n_fft, n_mels)
    assert lib.wt_mel_tables(24000, 1024, 100, None, None) == 0


def test_create_refuses_other_parameters_before_any_device_call():
    for sr, n_fft, hop, n_mels in ((24000, 512, 256, 100), (24000, 1024, 0, 100), (24000, 1024, 1025, 100), (24000, 1024, 256, 0),
                                   (24000, 1024, 256, 129), (1, 1024, 256, 100)):
        h = ctypes.c_void_p()
        assert lib.wt_mel_create(sr, n_fft, hop, n_mels, 0, ctypes.byref(h)) == WT_ERR_INVALID, (sr, n_fft, hop, n_mels)
        assert not h.value and lib.wt_last_error()
    assert lib.wt_mel_create(24000, 1024, 256, 100, 0, None) == WT_ERR_INVALID


def test_frames():
    h = fake_handle()
    want = {512: -1, 513: 3, 767: 3, 768: 4, 72000: 282}
    for T, f in want.items():
        assert lib.wt_mel_frames(ctypes.byref(h), T) == f, T
        if f > 0:
            assert metrics.mel_frames(T) == f == R.n_frames(T, 256)
    with pytest.raises(ValueError):
        metrics.mel_frames(512)
    assert lib.wt_mel_frames(None, 4096) == -1
    assert lib.wt_mel_frames(ctypes.byref(fake_handle(hop=100)), 3000) == 31
    assert lib.wt_mel_workspace_bytes(3, 10) == 48 * 3 + 40 and lib.wt_mel_workspace_bytes(0, 10) == 0


A, B_, OUT, WS = 0x7100000000, 0x7200000000, 0x7300000000, 0x7400000000


def _clips(n=1, **over):
    descs = (WtMelClip * n)()
    for i in range(n):
        descs[i].a, descs[i].b, descs[i].length, descs[i].out = A, B_, 3000, OUT
    for k, v in over.items():
        setattr(descs[n - 1], k, v)
    return descs


def _refused(call, what):
    assert call() == WT_ERR_INVALID, what
    msg = lib.wt_last_error().decode()
    assert msg.startswith("wt_mel_"), (what, msg)
    return msg


@pytest.mark.parametrize("distance", [False, True])
def test_every_refusal_is_made_before_any_device_call(distance):
    h = fake_handle()
    ws = ctypes.c_void_p(WS)

    def call(handle=h, clips=None, n=1, workspace=ws):
        hp = ctypes.byref(handle) if handle is not None else None
        clips = _clips(n) if clips is None else clips
        if distance:
            return lambda: lib.wt_mel_distance(hp, clips, n, workspace, None)
        return lambda: lib.wt_mel_spectrogram(hp, clips, n, 1, workspace, None)

    assert "null handle" in _refused(call(handle=None), "null handle")
    assert "null a" in _refused(call(clips=_clips(a=None)), "null a")
    assert "null out" in _refused(call(clips=_clips(out=None)), "null out")
    assert "clip 2: null a" in _refused(call(clips=_clips(3, a=None), n=3), "the last of three")
    assert "length" in _refused(call(clips=_clips(length=512)), "length 512")
    assert "length" in _refused(call(clips=_clips(length=0)), "length 0")
    assert "misaligned" in _refused(call(clips=_clips(a=A + 2)), "misaligned a")
    assert "misaligned" in _refused(call(clips=_clips(out=OUT + 1)), "misaligned out")
    assert "workspace" in _refused(call(workspace=ctypes.c_void_p(WS + 4)), "misaligned workspace")
    assert "workspace" in _refused(call(workspace=None), "null workspace")
    assert "B outside" in _refused(call(n=0), "B = 0")
    assert "B outside" in _refused(lambda: (lib.wt_mel_distance(ctypes.byref(h), _clips(1), 65536, ws, None) if distance else
                                            lib.wt_mel_spectrogram(ctypes.byref(h), _clips(1), 65536, 1, ws, None)), "B = 65536")
    if distance:
        assert "null b" in _refused(call(clips=_clips(b=None)), "null b")
        assert "misaligned" in _refused(call(clips=_clips(b=B_ + 2)), "misaligned b")
    else:
        clips = _clips(b=None)                                  # b is ignored: the call gets as far as the device check
        assert "another device" in _refused(call(clips=clips), "b ignored")
    # a sound call on a handle of device 63: refused for the device (no machine here has 64 GPUs and the last one current)
    assert "another device" in _refused(call(), "handle of another device")
    assert "another device" in _refused(call(n=70, clips=_clips(70)), "handle of another device, workspace path")
    assert "handle" in _refused(call(handle=fake_handle(hop=0)), "not a handle")


def test_python_surface_refuses_unequal_lengths_and_cpu_tensors():
    a, b = torch.zeros(3000), torch.zeros(3001)
    with pytest.raises(ValueError, match="lengths 3000 and 3001 differ"):
        metrics.mel_distance_many([a], [b])
    with pytest.raises(ValueError, match="as many"):
        metrics.mel_distance_many([a], [a, a])
    with pytest.raises(ValueError, match="shapes"):
        metrics.mel_distance(a, b)
    for call in (lambda: metrics.mel_distance_many([a], [a]), lambda: metrics.mel_distance(a, a), lambda: metrics.mel_spectrogram(a),
                 lambda: metrics.mel_spectrogram_many([a]), lambda: metrics.mel_spectrogram(torch.zeros(2, 1, 3000))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(ARCH_HOP600)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.round_trip_mel_distance([torch.zeros(12000)])
