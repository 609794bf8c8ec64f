"""The host side of the pitch / periodicity metrics (csrc/pitch.hip, wavtokenizer_amd/metrics.py) without a GPU: the exports, the
tables a handle uploads against the float64 definition (tests/pitch_ref.py), the frame counts, every refusal, made with fake
pointers and a fake handle of a device no test machine has current, so that nothing can ever be launched, and the float64
definition itself on signals whose answer is known."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import pitch_ref as R
from wavtokenizer_amd import _capi, metrics
from wavtokenizer_amd._capi import WT_ERR_INVALID, WtPitchClip, WtPitchPair, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PITCH_EXPORTS = {"wt_pitch_create", "wt_pitch_destroy", "wt_pitch_frames", "wt_pitch_tables", "wt_pitch_workspace_bytes",
                 "wt_pitch_track", "wt_pitch_pairs"}


class FakePitch(ctypes.Structure):
    """struct wt_pitch of csrc/pitch.hip."""
    _fields_ = [("device", ctypes.c_int), ("tab", ctypes.c_void_p)]


def fake_handle(device=63, tab=0x7000000000):
    h = FakePitch()
    h.device, h.tab = device, tab
    return h


def test_header_capi_and_library_agree_on_the_pitch_exports():
    header = open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")).read()
    declared = {s for s in re.findall(r"\b(wt_[a-z0-9_]+)\s*\(", header) if s.startswith("wt_pitch")}
    assert declared == PITCH_EXPORTS
    assert PITCH_EXPORTS <= set(_capi.EXPORTS)
    for sym in PITCH_EXPORTS:
        assert getattr(lib, sym) is not None
    assert ctypes.sizeof(WtPitchClip) == 32 and ctypes.sizeof(WtPitchPair) == 32


def test_tables_are_the_float64_definition_rounded_once():
    window, aw = np.full(R.WIN, np.nan, np.float32), np.full(R.BINS, np.nan, np.float32)
    assert lib.wt_pitch_tables(window.ctypes.data_as(ctypes.c_void_p), aw.ctypes.data_as(ctypes.c_void_p)) == 0
    for got, want64 in ((window, R.window64()), (aw, R.a_weighting64())):
        want = want64.astype(np.float32)
        # (two float64 cosines or logarithms may differ in their last bit, which can move the one rounding to fp32 by an ulp at a near-tie)
        assert bool((np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all())
    assert float(np.abs(torch.hann_window(R.WIN, periodic=True, dtype=torch.float64).numpy() - R.window64()).max()) < 1e-15
    assert window[0] == 0 and window[R.WIN // 2] == 1 and bool((window[1:] > 0).all())
    assert aw[0] == -80 and bool((aw >= -80).all())
    assert abs(float(aw[64])) < 0.01                             # bin 64 is 1 kHz: the A-weighting's reference point
    assert abs(float(aw[128]) - 1.2) < 0.01 and -22.0 < float(aw[6]) < -19.1          # IEC 61672: +1.2 dB at 2 kHz, -19.1 at 100 Hz (bin 6: 93.75 Hz)
    assert lib.wt_pitch_tables(None, None) == 0


def test_frames_and_workspace():
    for T, n in ((0, 0), (1023, 0), (1024, 1), (1183, 1), (1184, 2), (48000, 294), (1024 + 160 * 63, 64)):
        assert lib.wt_pitch_frames(T) == n == metrics.pitch_frames(T) == R.n_frames(T), T
    assert lib.wt_pitch_workspace_bytes(3, 10) == 144 + 4 * (100 + 6)     # 3 descriptors of 48 bytes, ten floats per frame, two per clip
    assert lib.wt_pitch_workspace_bytes(0, 10) == 0 and lib.wt_pitch_workspace_bytes(3, -1) == 0


X, Y, OUT, TAPS, WS = 0x7100000000, 0x7200000000, 0x7300000000, 0x7500000000, 0x7400000000


def _clips(pairs, n=1, **over):
    descs = ((WtPitchPair if pairs else WtPitchClip) * n)()
    for i in range(n):
        if pairs:
            descs[i].reference, descs[i].estimate, descs[i].length, descs[i].out = X, Y, 3000, OUT
        else:
            descs[i].signal, descs[i].length, descs[i].out, descs[i].taps = X, 3000, OUT, TAPS
    for k, v in over.items():
        setattr(descs[n - 1], k, v)
    return descs


@pytest.mark.parametrize("pairs", [False, True])
def test_every_refusal_is_made_before_any_device_call(pairs):
    h = fake_handle()
    ws = ctypes.c_void_p(WS)
    name = "wt_pitch_pairs" if pairs else "wt_pitch_track"
    first = "reference" if pairs else "signal"

    def call(handle=h, clips=None, n=1, workspace=ws, thr=(0.15, -60.0, 0.5)):
        hp = ctypes.byref(handle) if handle is not None else None
        clips = _clips(pairs, n) if clips is None else clips
        return lambda: getattr(lib, name)(hp, clips, n, *thr, workspace, None)

    def refused(c, what):
        assert c() == WT_ERR_INVALID, what
        msg = lib.wt_last_error().decode()
        assert msg.startswith(name), (what, msg)
        return msg

    assert "null handle" in refused(call(handle=None), "null handle")
    assert "null clips" in refused(lambda: getattr(lib, name)(ctypes.byref(h), None, 1, 0.15, -60.0, 0.5, ws, None), "null clips")
    assert "null " + first in refused(call(clips=_clips(pairs, **{first: None})), "null signal")
    assert "null out" in refused(call(clips=_clips(pairs, out=None)), "null out")
    assert "2: null " + first in refused(call(clips=_clips(pairs, 3, **{first: None}), n=3), "the last of three")
    assert "length" in refused(call(clips=_clips(pairs, length=1023)), "length 1023")
    assert "length" in refused(call(clips=_clips(pairs, length=0)), "length 0")
    assert "misaligned" in refused(call(clips=_clips(pairs, **{first: X + 2})), "misaligned signal")
    assert "misaligned" in refused(call(clips=_clips(pairs, out=OUT + 1)), "misaligned out")
    assert "workspace" in refused(call(workspace=ctypes.c_void_p(WS + 4)), "misaligned workspace")
    assert "workspace" in refused(call(workspace=None), "null workspace")
    assert "B outside" in refused(call(n=0), "B = 0")
    assert "B outside" in refused(call(n=65536, clips=_clips(pairs, 1)), "B = 65536")
    assert "NaN" in refused(call(thr=(float("nan"), -60.0, 0.5)), "NaN threshold")
    if pairs:
        assert "null estimate" in refused(call(clips=_clips(pairs, estimate=None)), "null estimate")
        assert "misaligned" in refused(call(clips=_clips(pairs, estimate=Y + 2)), "misaligned estimate")
    else:
        assert "misaligned" in refused(call(clips=_clips(pairs, taps=TAPS + 2)), "misaligned taps")
        assert "another device" in refused(call(clips=_clips(pairs, taps=None)), "taps are optional")
    # the order is stftd_run's: the call's own arguments, then the clips in order, then the device
    assert "null handle" in refused(call(handle=None, workspace=None, n=0), "handle first")
    assert "workspace" in refused(call(workspace=None, n=0), "then clips and workspace")
    assert "B outside" in refused(call(n=0, clips=_clips(pairs, out=None)), "then B")
    assert "null out" in refused(call(clips=_clips(pairs, out=None, length=0)), "a clip's pointers before its length")
    assert "length" in refused(call(clips=_clips(pairs, length=0, out=OUT + 1)), "its length before its alignment")
    # a sound call on a handle of device 63: refused for the device (no machine here has 64 GPUs and the last one current)
    assert "another device" in refused(call(), "handle of another device")
    assert "another device" in refused(call(clips=_clips(pairs, length=1024)), "one frame is enough")
    assert "another device" in refused(call(n=70, clips=_clips(pairs, 70)), "handle of another device, workspace path")
    assert "handle" in refused(call(handle=fake_handle(tab=0)), "not a handle")
    assert lib.wt_pitch_create(0, None) == WT_ERR_INVALID and lib.wt_last_error().decode().startswith("wt_pitch_create")


def test_python_surface_checks_its_arguments():
    a, b = torch.zeros(3000), torch.zeros(3001)
    with pytest.raises(ValueError, match="lengths 3000 and 3001 differ"):
        metrics.periodicity_metrics_many([a], [b])
    with pytest.raises(ValueError, match="lengths 3000 and 3001 differ"):
        metrics.periodicity_metrics(a, b)
    with pytest.raises(ValueError, match="as many"):
        metrics.periodicity_metrics_many([a], [a, a])
    for call in (lambda: metrics.pitch(a[:1023]), lambda: metrics.pitch_many([a, a[:1023]]), lambda: metrics.periodicity_metrics(a[:1023], a[:1023]),
                 lambda: metrics.pitch(a[:1534], 24000), lambda: metrics.periodicity_metrics_many([a, a[:2000]], [a, a[:2000]], sample_rate=[16000, 48000])):
        with pytest.raises(ValueError, match="too short"):
            call()
    for call in (lambda: metrics.pitch(a.to(torch.int16)), lambda: metrics.periodicity_metrics(a, a.to(torch.int32)),
                 lambda: metrics.pitch_many([a, a.to(torch.int16)])):
        with pytest.raises(ValueError, match="floating-point"):
            call()
    with pytest.raises(ValueError, match="1-D"):
        metrics.pitch(torch.zeros(2, 3000))
    with pytest.raises(ValueError, match="1-D"):
        metrics.periodicity_metrics_many([torch.zeros(2, 3000)], [torch.zeros(2, 3000)])
    with pytest.raises(ValueError, match="one per clip"):
        metrics.pitch_many([a, a], sample_rate=[16000])
    with pytest.raises(ValueError, match="positive integer"):
        metrics.pitch(a, 16000.5)
    with pytest.raises(ValueError, match="NaN"):
        metrics.pitch(a, threshold=float("nan"))
    assert metrics.pitch_many([]) == [] and metrics.pitch_frames(1536) == 4
    # a tensor that is not on the GPU: this package's wording for it, as every other metric here
    for call in (lambda: metrics.pitch(a), lambda: metrics.pitch_many([a]), lambda: metrics.periodicity_metrics(a, a),
                 lambda: metrics.periodicity_metrics_many([a], [a]), lambda: metrics.pitch(a[:1536], 24000)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(ARCH_HOP600)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.round_trip_periodicity([torch.zeros(12000)])


# ------------------------------------------------------------------------------------------------ the float64 definition itself
@pytest.mark.parametrize("freq", [50.5, 60.0, 100.0, 440.0, 530.0])
def test_reference_finds_pure_tones(freq):
    t = R.Track(R.tone(freq))
    cents = np.abs(1200.0 * np.log2(t.f0_raw / freq))
    assert t.n == 19 and float(cents.max()) < 1.5 and float(t.per_raw.min()) > 0.999, (cents.max(), t.per_raw.min())
    assert bool((t.per == t.per_raw).all()) and not np.isnan(t.f0).any()           # loud and periodic: voiced throughout


def test_reference_gives_a_tone_above_the_range_as_its_subharmonic():
    t = R.Track(R.tone(1000.0))
    assert float(np.abs(1200.0 * np.log2(t.f0_raw / 500.0)).max()) < 1.5 and float(t.per_raw.min()) > 0.999


@pytest.mark.parametrize("level", [0.0, 0.25])
def test_reference_on_silence_and_dc(level):
    x = np.full(4000, level, np.float32)
    t = R.Track(x)
    assert bool((t.per_raw == 0).all()) and bool((t.per == 0).all()) and np.isnan(t.f0).all()
    assert bool((t.f0_raw == R.RATE / R.LAG_LO).all())             # d' is 1 everywhere: the smallest lag of the range, no offset
    m = R.periodicity_metrics64(x, x)
    assert m[0] == 0 and np.isnan(m[1]) and np.isnan(m[2])
    if level == 0.0:
        assert bool((t.loud < -60).all())                           # -100 dB in every bin


def test_reference_pair_formulas_and_their_nan():
    nan = np.nan
    f0, per = np.array([100.0, nan, 200.0, nan]), np.array([0.9, 0.1, 0.8, 0.0])
    g0, qer = np.array([100.0 * 2 ** (30 / 1200), 150.0, nan, nan]), np.array([0.9, 0.6, 0.2, 0.0])
    m = R.pair_metrics(f0, per, g0, qer)
    assert abs(m[0] - np.sqrt((0.5 ** 2 + 0.6 ** 2) / 4)) < 1e-15 and abs(m[1] - 30.0) < 1e-9 and abs(m[2] - 0.5) < 1e-15       # TP 1, FP 1, FN 1
    assert np.isnan(R.pair_metrics(f0, per, np.full(4, nan), qer)[1:]).all()         # no voiced estimate frame: precision 0 / 0
    both_zero = R.pair_metrics(np.array([100.0, nan]), per[:2], np.array([nan, 100.0]), per[:2])
    assert np.isnan(both_zero[1]) and np.isnan(both_zero[2])                          # precision = recall = 0: 0 / 0 in the F1


def test_reference_recipe_moves_all_three_outputs():
    """The test clip of the GPU tests: silent, noisy and voiced frames, and a decoded twin at 30 and 0 dB that moves the metrics."""
    x = R.recipe(16000, 0)
    t = R.Track(x)
    silent, voiced = float((t.loud < R.SILENCE).mean()), float((~np.isnan(t.f0)).mean())
    assert 0.05 < silent < 0.25 and 0.5 < voiced < 0.8, (silent, voiced)
    good, bad = R.periodicity_metrics64(x, R.decoded(x, 30, 0)), R.periodicity_metrics64(x, R.decoded(x, 0, 0))
    assert good[2] == 1.0 and good[1] < 1.0 and good[0] < 0.06
    assert 0.8 < bad[2] < 0.99 and bad[1] > 100.0 and bad[0] > 0.2


# ------------------------------------------------------------------------------------------------ what tests/test_pitch_range.py rests on
def test_reference_recipe_clips_show_no_frame_opened_by_the_den_decision_alone():
    c = R.cases()
    assert c.new_den_open == [0] * len(c.signals) and min(float(np.abs(t.den).min()) for t in c.t64) > 10 * R.DEN_GUARDS * c.guard
    assert c.standin_flips_covered and max(c.open_fraction) <= R.OPEN_CAP


def test_reference_sweep_reaches_every_lag_with_a_sure_frame():
    s, c = R.sweep(), R.cases()
    t, sure = s.t64, s.sure
    assert t.n == 591 and set(t.lag[sure].tolist()) == set(range(R.LAG_LO, R.LAG_HI + 1))           # 291 distinct sure lags
    assert int((sure & (t.lag == R.LAG_HI)).sum()) >= 5 and int((sure & (t.lag == R.LAG_LO)).sum()) >= 2
    assert int((sure & (t.off == 0.5)).sum()) >= 5 and float(s.open.mean()) <= R.OPEN_CAP
    assert tuple(t.lag[:2]) == (58, 59)                             # periods 28.8 and 29.3: under the range, found as their subharmonics
    assert not s.flipped.any() and s.standin_flips_covered and s.pool_den_flips_covered
    # the stand-in errs no more here than on the recipe clips: the YIN taps, whose arithmetic is numpy's own.  The loudness stand-in
    # is the platform's fp32 FFT, and the largest of some hundred frames' errors lands on either side of the recipe clips' from one
    # CPU to the next (1.005 and 1.29 times it on two machines): there the bar is held to the smaller of the two instead (EdgeSet)
    assert s.standin[0] <= c.standin[0] and s.standin[1] <= c.standin[1], (s.standin, c.standin)
    assert bool((s.bar_base <= np.array(c.standin)).all()) and bool((s.bar_base <= np.array(s.standin)).all())


def test_reference_low_tones_take_both_clamps_and_the_den_not_positive_branch():
    s, c = R.low_tones(), R.cases()
    t = s.t64
    assert s.pool_n == 1080 and t.n >= 100 and bool(s.sure.all())
    assert int((t.den < 0).sum()) >= 30 and int((t.off == 0.5).sum()) >= 20 and int((t.off == -0.5).sum()) >= 20
    assert bool((t.off[t.den < 0] == 0).all()) and bool(((t.den < 0) | (np.abs(t.off) == 0.5)).all())
    assert set(t.lag.tolist()) == {R.LAG_LO, R.LAG_HI} and bool(t.fallback.all())
    assert not s.flipped.any() and s.standin_flips_covered
    # the pool is where the stand-in's den falls on the other side of 0: every such frame lies inside the den guard, and so is left out
    assert int(s.pool_den_flips.sum()) >= 1 and s.pool_den_flips_covered and s.pool_den_near > s.pool_n // 2
    assert s.standin[0] <= c.standin[0] and s.standin[1] <= c.standin[1], (s.standin, c.standin)           # (the loudness: as above)
    assert bool((s.bar_base <= np.array(c.standin)).all()) and bool((s.bar_base <= np.array(s.standin)).all())


def test_reference_den_decision_gives_the_answers_on_both_sides():
    """A d' that falls in a straight line to lag 320, as under a tone below the range, bent by 1e-6 at lag 321 either way: float64
    gives the clamp or off = 0, the frame is den_open, and it is held against off = 0 and the clamp on the side of a - c alone."""
    c = R.cases()
    for eps, off64 in ((1e-6, 0.5), (-1e-6, 0.0), (0.0, 0.0)):
        dp = (1.5 - 0.002 * np.arange(R.MAX_LAG + 1))[None, :].copy()
        dp[0, R.MAX_LAG] += eps
        t = R.Track((np.float64, dp, np.zeros(1)), np.float64, R.THRESHOLD, **R.EVERY)
        assert t.lag[0] == R.LAG_HI and t.fallback[0] and t.off[0] == off64 and abs(t.den[0] - eps) < 1e-12
        lag_open, gate_open, den_open = R.decisions(t, c.guard, c.guard_db, R.THRESHOLD, **R.EVERY)
        assert den_open[0] and not lag_open[0] and not gate_open[0]
        for off, ok in ((0.0, True), (0.5, True), (-0.5, False), (0.25, False)):
            f0, per = R.from_offset(t.lag, dp[:, 319], dp[:, 320], dp[:, 321], off)
            e = R.tap_errors(f0, per, t.loud, t, lag_open, den_open, c.guard)
            assert (e[0] < 1e-12 and e[1] < 1e-9) == ok and R.admissible(f0, per, 0, t, c.guard, c.bar_per, c.bar_cents) == ok, (eps, off, e)
        if off64:                                                   # without the den decision the clamp is the one answer
            f0, per = R.from_offset(t.lag, dp[:, 319], dp[:, 320], dp[:, 321], 0.0)
            assert R.tap_errors(f0, per, t.loud, t, lag_open)[1] > 2.0            # 2.7 cents at lag 320
    # a - c within its guard as well: the quotient of two open numbers, any offset in [-0.5, 0.5], pitch and periodicity from one
    dp = np.full((1, R.MAX_LAG + 1), 0.9)
    dp[0, R.LAG_LO - 1:R.LAG_LO + 2] = (0.80006, 0.8, 0.80005)
    t = R.Track((np.float64, dp, np.zeros(1)), np.float64, R.THRESHOLD, **R.EVERY)
    lag_open, _, den_open = R.decisions(t, c.guard, c.guard_db, R.THRESHOLD, **R.EVERY)
    assert t.lag[0] == R.LAG_LO and den_open[0] and not lag_open[0]
    for off in (-0.5, -0.2, 0.0, 0.37, 0.5):
        f0, per = R.from_offset(t.lag, dp[:, R.LAG_LO - 1], dp[:, R.LAG_LO], dp[:, R.LAG_LO + 1], off)
        e = R.tap_errors(f0, per, t.loud, t, lag_open, den_open, c.guard)
        assert e[0] < 1e-12 and e[1] < 1e-9, (off, e)
        assert R.tap_errors(f0, per + 1e-4, t.loud, t, lag_open, den_open, c.guard)[0] > 9e-5


@pytest.mark.parametrize("setting", R.SETTINGS)
def test_reference_threshold_grid_keeps_the_open_frames_under_the_cap(setting):
    c = R.cases_at(setting)
    assert max(c.open_fraction) <= R.OPEN_CAP, c.open_fraction
    assert c.standin_flips_covered and c.guard == R.cases().guard
    threshold, silence, unvoiced = setting
    if threshold == 0.0:
        assert all(bool(t.fallback.all()) for t in c.t64)
    if threshold == 10.0:
        assert not any(bool(t.fallback.any()) for t in c.t64) and int(((c.t64[3].lag == R.LAG_LO) & ~c.open[3]).sum()) >= 5
    if setting == (0.15, -40.0, 0.21):
        assert float((c.t64[0].loud < silence).mean()) > 0.5
    if unvoiced == 1.0:
        assert all(bool(np.isnan(t.f0).all()) for t in c.t64)
        assert all(np.isnan(R.pair_metrics(c.t64[i].f0, c.t64[i].per, c.t64[j].f0, c.t64[j].per)[1:]).all() for i, j in c.pairs)


def test_reference_pair_with_precision_and_recall_zero():
    c = R.cases()
    ref, est = R.pr_zero_pair()
    a, b = R.Track(ref), R.Track(est)
    va, vb = ~np.isnan(a.f0), ~np.isnan(b.f0)
    assert not any(np.logical_or.reduce(R.decisions(t, c.guard, c.guard_db)).any() for t in (a, b))
    assert a.n == 34 and int((va & vb).sum()) == 0 and int((~va & vb).sum()) > 0 and int((va & ~vb).sum()) > 0
    m = R.pair_metrics(a.f0, a.per, b.f0, b.per)
    assert m[0] > 0.5 and np.isnan(m[1]) and np.isnan(m[2])


def test_reference_tie_clips_rest_on_the_left_neighbour_being_allowed_to_tie():
    x = np.stack([R.tie_clip(lag) for lag in R.TIE_LAGS])
    for dtype in (np.float64, np.float32):
        t = R.Track(x, dtype, threshold=10.0, one_frame_clips=True, **R.EVERY)
        assert tuple(t.lag) == R.TIE_LAGS and not t.fallback.any() and bool((t.off == -0.5).all()) and bool((t.per_raw == 1).all())
        for k, lag in enumerate(R.TIE_LAGS):
            assert bool((t.dp[k, 1:lag + 1] == 1).all()) and t.dp[k, lag + 1] == lag + 1 and bool((np.diff(t.dp[k, lag + 1:]) < 0).all())
        strict = R.candidates(t.dp, dtype(10.0)) & (t.dp[:, R.LAG_LO:R.LAG_HI + 1] < t.dp[:, R.LAG_LO - 1:R.LAG_HI])
        assert not strict.any()                                     # with < on the left there is no candidate at all: lag 30 by the fallback
