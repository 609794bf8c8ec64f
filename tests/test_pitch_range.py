"""The pitch kernels (csrc/pitch.hip) over their whole range, through ctypes as in tests/test_pitch_op.py: every searchable lag, the
two ends of the range with the parabola's clamp and its den <= 0 branch, every wave slot of the workgroup, a grid of thresholds, the
F1 with precision = recall = 0, and gains to 2^15 and 2^-40, against the float64 definition (tests/pitch_ref.py).

The signals are edge_tone() clips of one frame each: the sweep (591 periods 28.8 .. 323.8, every lag 30 .. 320 picked by a sure
frame) and the low tones (periods 321 .. 1400, under the search range: the pool members whose float64 frame is sure under every
guard), and the recipe clips of tests/test_pitch_op.py at other thresholds.  Per set, a bar is 4 x what the fp32 stand-in of
tests/pitch_ref.py reaches on that set against float64, never over the recipe clips' bar and never under 4 half-units of fp32 at
the value; the guards are the recipe clips'.  A frame whose den = a - 2 b + c lies within 4 guards of 0 is held against off = 0,
float64's offset and the clamp on the side of a - c, whichever is nearest.  tests/test_pitch_host.py asserts on the CPU what these
tests rest on.  Measured on an MI355X: profiles/pitch_range_error.txt."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import pitch_ref as R

pytestmark = pytest.mark.gpu


def _hold(name, s, got):
    """One-frame clips of an EdgeSet against float64: every sure frame within the set's bars, every open one an admissible answer."""
    f0, raw, loud = (np.array([g[k][0] for g in got]) for k in (0, 2, 3))
    assert all(len(g[0]) == 1 for g in got) and not np.isnan(f0).any() and not np.isnan(raw).any() and not np.isnan(loud).any()
    assert np.array_equal(np.array([g[1][0] for g in got]), raw)                   # nothing is gated in this call
    err, bars = s.errors(f0, raw, loud)
    print(f"pitch_range {name}: n {s.t64.n}  open {int(s.open.sum())}  stand-in {s.standin[0]:.3e} {s.standin[1]:.3e} {s.standin[2]:.3e}")
    for k, what in enumerate(("periodicity", "cents", "loudness dB")):
        w = int((err[k] / bars[k]).argmax())
        print(f"pitch_range {name}: {what:12s} worst {err[k].max():.3e}  nearest its bar at clip {w}: {err[k][w]:.3e} (bar {bars[k][w]:.3e})")
    bad = [(int(f), err[:, f], bars[:, f]) for f in np.nonzero((err > bars).any(axis=0))[0]]
    assert not bad, bad[:5]
    assert not s.not_admissible(f0, raw)
    return f0, raw


def test_every_lag_against_float64():
    s = R.sweep()
    got, intact = R.run_track(s.signals, **R.EVERY)                 # 591 clips: descriptors through the workspace
    assert intact
    f0, _ = _hold("sweep", s, got)
    # what the kernel itself returned on the sure frames: every lag of the range (its period less float64's offset, rounded)
    lags = np.rint(R.RATE / f0.astype(np.float64) - s.t64.off).astype(int)
    assert set(lags[s.sure].tolist()) == set(range(R.LAG_LO, R.LAG_HI + 1))
    assert np.array_equal(lags[s.sure], s.t64.lag[s.sure])
    clamped = s.sure & (s.t64.off == 0.5)                           # periods past 320.5: lag 320 through the fallback, off in its clamp
    assert np.array_equal(f0[clamped], (np.float32(R.RATE) / (s.t64.lag[clamped].astype(np.float32) + np.float32(0.5))))


def test_range_edges_clamp_and_den_not_positive():
    s = R.low_tones()
    got, intact = R.run_track(s.signals, **R.EVERY)
    assert intact
    f0, _ = _hold("low tones", s, got)
    t = s.t64
    assert bool(t.fallback.all()) and set(t.lag.tolist()) == {R.LAG_LO, R.LAG_HI} and bool(s.sure.all())
    # the offset is 0 (den <= 0) or in its clamp: the pitch is one fp32 division of exact operands
    assert bool(((t.den < 0) | (np.abs(t.off) == 0.5)).all())
    want = np.float32(R.RATE) / (t.lag.astype(np.float32) + t.off.astype(np.float32))
    wrong = np.nonzero(f0 != want)[0]
    assert len(wrong) == 0, [(int(k), float(f0[k]), float(want[k]), float(t.den[k])) for k in wrong[:5]]


def test_lane_and_wave_placement():
    """Sweep clips of lags 30, 35 and 320 as the last frame of clips of 1, 2, 3 and 4 frames: every wave slot of the workgroup, the
    rest of it idle, gives the bits of the one-frame call."""
    s = R.sweep()
    picks = [int(np.nonzero(s.sure & (s.t64.lag == lag))[0][0]) for lag in (R.LAG_LO, 35, R.LAG_HI)]
    head = R.cases().signals[0][3000:3000 + 3 * R.HOP]
    clips = [np.concatenate([head[:R.HOP * m], s.signals[k]]) for k in picks for m in range(4)]
    got, intact = R.run_track(clips, **R.EVERY)
    assert intact and [len(g[0]) for g in got] == [1, 2, 3, 4] * 3
    for i, k in enumerate(picks):
        one = got[4 * i]
        assert abs(1200.0 * np.log2(float(one[0][0]) / s.t64.f0_raw[k])) <= R.BAR_FACTOR * max(s.standin[1], 1200.0 / np.log(2.0) * R.HALF_UNIT)
        for m in range(1, 4):
            g = got[4 * i + m]
            assert g[0][-1] == one[0][0] and g[2][-1] == one[2][0], (s.t64.lag[k], m, g[0][-1], one[0][0], g[2][-1], one[2][0])


def test_a_tie_with_the_left_neighbour_is_a_candidate():
    """tie_clip(): d'(lag - 1) = d'(lag) = 1 < d'(lag + 1), every number exact in fp32 as in float64, so no guard applies: the lag is
    the candidate (<= on the left), the pitch is 16000 / (lag - 0.5) to the bit and the periodicity 1."""
    clips = [R.tie_clip(lag) for lag in R.TIE_LAGS]
    t = R.Track(np.stack(clips), threshold=10.0, one_frame_clips=True, **R.EVERY)
    assert tuple(t.lag) == R.TIE_LAGS and bool((t.off == -0.5).all()) and bool((t.per_raw == 1).all()) and not t.fallback.any()
    got, intact = R.run_track(clips, 10.0, **R.EVERY)
    assert intact
    for lag, (f0, per, raw, loud) in zip(R.TIE_LAGS, got):
        assert f0[0] == np.float32(R.RATE) / (np.float32(lag) - np.float32(0.5)) and raw[0] == 1 and per[0] == 1, (lag, f0, raw)


@pytest.mark.parametrize("setting", R.SETTINGS, ids=lambda s: "thr{}_sil{}_unv{}".format(*s))
def test_threshold_grid_against_float64(setting):
    """The recipe clips of tests/test_pitch_op.py at another (threshold, silence, unvoiced): the taps, the gate and the voicing and
    the pair metrics against the float64 references at that setting."""
    base, c = R.cases(), R.cases_at(setting)
    threshold, silence, unvoiced = setting
    print(f"pitch_range setting {setting}: stand-in {c.standin[0]:.3e} {c.standin[1]:.3e} {c.standin[2]:.3e}  pair {c.standin_pair}  "
          f"open {[int(o.sum()) for o in c.open]}")
    assert c.standin_flips_covered and max(c.open_fraction) <= R.OPEN_CAP and base.new_den_open == [0] * len(base.signals)
    # what the setting is there for, from float64 alone
    if threshold == 0.0:
        assert all(bool(t.fallback.all()) for t in c.t64)
    if threshold == 10.0:
        assert not any(bool(t.fallback.any()) for t in c.t64)
        assert int(((c.t64[3].lag == R.LAG_LO) & ~c.open[3]).sum()) >= 5          # signal 3: a twin at 0 dB
    if setting == (0.15, -40.0, 0.21):
        assert float((c.t64[0].loud < silence).mean()) > 0.5
    if unvoiced == 1.0:
        assert all(bool(np.isnan(t.f0).all()) for t in c.t64)
    tracks, intact = R.run_track(c.signals, threshold, silence, unvoiced)
    every, intact2 = R.run_track(c.signals, threshold, **R.EVERY)
    assert intact and intact2
    bad = []
    for i, ((f0, per, raw, loud), t) in enumerate(zip(tracks, c.t64)):
        # the taps (tests/test_pitch_op.py: test_taps_against_float64)
        f0_raw = every[i][0]
        assert f0.shape == (t.n,) and not np.isnan(raw).any() and not np.isnan(loud).any() and not np.isnan(per).any(), i
        assert not np.isnan(f0_raw).any() and np.array_equal(every[i][2], raw) and np.array_equal(every[i][3], loud), i
        assert np.array_equal(every[i][1], raw) and np.array_equal(f0[~np.isnan(f0)], f0_raw[~np.isnan(f0)]), i
        e = R.tap_errors(f0_raw, raw, loud, t, c.lag_open[i], c.den_open[i], c.guard)
        print(f"pitch_range setting {setting} signal {i}  periodicity {e[0]:.3e} (bar {c.bar_per:.3e})  cents {e[1]:.3e} (bar {c.bar_cents:.3e})  "
              f"loudness {e[2]:.3e} dB (bar {c.bar_db:.3e})  open {int(c.open[i].sum())}")
        if not (e[0] <= c.bar_per and e[1] <= c.bar_cents and e[2] <= c.bar_db):
            bad.append((i, e))
        for f in np.nonzero(c.lag_open[i] | c.den_open[i])[0]:
            if not R.admissible(f0_raw, raw, f, t, c.guard, c.bar_per, c.bar_cents, threshold):
                bad.append((i, int(f), "not an admissible answer"))
        # the gate and the voicing (test_gate_and_voicing_follow_the_float64_decisions)
        silent, voiced = loud < np.float32(silence), ~np.isnan(f0)
        assert np.array_equal(per, np.where(silent, np.float32(0), raw)) and np.array_equal(voiced, per >= np.float32(unvoiced)), i
        sure = ~c.open[i]
        assert np.array_equal(silent[sure], (t.loud < silence)[sure]) and np.array_equal(voiced[sure], ~np.isnan(t.f0)[sure]), i
        if (sure & voiced).any():
            cents = 1200.0 * np.log2(f0[sure & voiced].astype(np.float64) / t.f0[sure & voiced])
            assert float(np.abs(cents).max()) <= c.bar_cents, i
    assert not bad, bad
    # the pairs (test_pairs_against_float64)
    got, intact = R.run_pairs([c.signals[i] for i, _ in c.pairs], [c.signals[j] for _, j in c.pairs], threshold, silence, unvoiced)
    assert intact
    for (i, j), g in zip(c.pairs, got):
        want = c.pair_want(i, j, *(SimpleNamespace(f0=tracks[k][0], per=tracks[k][1]) for k in (i, j)))
        err, bar = R.metric_error(g, want), c.pair_bar(want)
        print(f"pitch_range setting {setting} pair ({i}, {j})  got {g}  float64 {want}  error {err}  (bar {bar})")
        if not bool((err <= bar).all()):
            bad.append(((i, j), err, bar))
        if unvoiced == 1.0:
            assert np.isnan(g[1]) and np.isnan(g[2]) and np.isnan(want[1]) and np.isnan(want[2])
    assert not bad, bad


def test_f1_with_precision_and_recall_zero():
    """A reference voiced only where the estimate is not: TP = 0 with FP > 0 and FN > 0, so precision = recall = 0 and the F1 is
    0 / 0; no frame is voiced in both, so the pitch loss is 0 / 0 as well."""
    c = R.cases()
    ref, est = R.pr_zero_pair()
    a, b = R.Track(ref), R.Track(est)
    opened = [np.logical_or.reduce(R.decisions(t, c.guard, c.guard_db)) for t in (a, b)]
    va, vb = ~np.isnan(a.f0), ~np.isnan(b.f0)
    assert not opened[0].any() and not opened[1].any()              # every decision of the pair is sure in float64
    assert int((va & vb).sum()) == 0 and int((~va & vb).sum()) > 0 and int((va & ~vb).sum()) > 0
    want = R.pair_metrics(a.f0, a.per, b.f0, b.per)
    assert np.isnan(want[1]) and np.isnan(want[2]) and want[0] > 0.5
    (got,), intact = R.run_pairs([ref], [est])
    assert intact and np.isnan(got[1]) and np.isnan(got[2]), got
    bar = c.pair_bar(want)
    print(f"pitch_range P = R = 0: got {got}  float64 {want}  error {abs(float(got[0]) - want[0]):.3e}  (bar {bar[0]:.3e})")
    assert abs(float(got[0]) - want[0]) <= bar[0]


def test_gain_to_int16_scale_and_far_down_moves_no_bit_of_the_yin_taps():
    """d scales by the gain's square exactly and stays in the normal range (d <= 703 (2 * 0.6 * 2^15)^2 at the top; at 2^-40 the
    noise floor's differences are still far over 2^-126), so d', the lag, the pitch and the ungated periodicity keep every bit."""
    x = R.cases().signals[0]
    gains = (4.0, 0.125, 2.0 ** 15, 2.0 ** -40)
    got, ok = R.run_track([x] + [x * np.float32(g) for g in gains], **R.EVERY)
    assert ok and not np.isnan(got[0][0]).any()
    for g, gain in zip(got[1:], gains):
        assert np.array_equal(g[2], got[0][2]) and np.array_equal(g[0], got[0][0]), gain
    assert float(np.abs(got[3][3] - got[0][3] - 20 * np.log10(2.0 ** 15)).max()) < 1e-3          # the loudness moves by the gain, floor included
    assert bool((got[4][3] < -100).all())                           # every bin under the 1e-10 floor: -100 dB + A - 20 in the mean
