"""The pitch kernels (csrc/pitch.hip) alone, through ctypes: clips in a NaN-filled arena, outputs and taps between canaries, the
workspace pre-filled, against the float64 definition (tests/pitch_ref.py).

The bars are measured, never taken from the kernel: per tap (ungated periodicity, f0 in cents, loudness in dB) 4 x what the fp32
stand-in of tests/pitch_ref.py reaches against float64 on the same signals on the CPU (the factor covers a different but fixed
summation order).  A frame whose float64 margin to a decision (d' against the threshold or a neighbour, a tie of the fallback
minimum, the parabola's den against 0, the periodicity against unvoiced_threshold, the loudness against silence_threshold) lies
inside a guard of 10 x the bar (4 guards for den, a sum of three d') may come out either way: it is held against the admissible
answers only, and the float64 pair metrics take the kernel's decisions at such frames.  At most 2 % of a clip's frames may be treated so: above that the test fails.
Measured on an MI355X: profiles/pitch_error.txt."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import pitch_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    c = R.cases()
    print(f"pitch stand-in (fp32, CPU): periodicity {c.standin[0]:.3e}  cents {c.standin[1]:.3e}  loudness {c.standin[2]:.3e} dB;"
          f" bars {c.bar_per:.3e} {c.bar_cents:.3e} {c.bar_db:.3e}; guards {c.guard:.3e} {c.guard_db:.3e} dB")
    print(f"pitch stand-in pair errors {c.standin_pair}; open frames per signal {[int(o.sum()) for o in c.open]} of {[t.n for t in c.t64]}")
    # (the yardstick itself: a few units of 2^-23 on d' near 0..1, and a transform error far under a thousandth of a dB)
    assert 1e-7 < c.standin[0] < 1e-5 and c.standin[1] < 0.05 and 1e-7 < c.standin[2] < 1e-3
    assert c.standin_flips_covered                                  # the stand-in itself changes its mind at open frames only
    assert max(c.open_fraction) <= R.OPEN_CAP, c.open_fraction
    assert c.new_den_open == [0] * len(c.signals)                   # the sign of the parabola's den is open at no frame of its own
    return c


@pytest.fixture(scope="module")
def tracks(cases):
    got, intact = R.run_track(cases.signals)                        # 8 clips: one call
    assert intact
    return got


def test_taps_against_float64(cases, tracks):
    # the pitch of every frame, voiced or not: a call in which no frame is silent or unvoiced; its taps are the other call's
    every, intact = R.run_track(cases.signals, silence=-1e30, unvoiced=-1.0)
    assert intact
    bad = []
    for i, ((f0, per, raw, loud), t) in enumerate(zip(tracks, cases.t64)):
        assert f0.shape == (t.n,) and not np.isnan(raw).any() and not np.isnan(loud).any() and not np.isnan(per).any(), i
        f0_raw = every[i][0]
        assert not np.isnan(f0_raw).any() and np.array_equal(every[i][2], raw) and np.array_equal(every[i][3], loud), i
        assert np.array_equal(every[i][1], raw) and np.array_equal(f0[~np.isnan(f0)], f0_raw[~np.isnan(f0)]), i
        e = R.tap_errors(f0_raw, raw, loud, t, cases.lag_open[i])
        print(f"pitch_error signal {i} T {len(cases.signals[i]):5d} n {t.n:3d}  periodicity {e[0]:.3e} (bar {cases.bar_per:.3e})  "
              f"cents {e[1]:.3e} (bar {cases.bar_cents:.3e})  loudness {e[2]:.3e} dB (bar {cases.bar_db:.3e})  open {int(cases.open[i].sum())}")
        if not (e[0] <= cases.bar_per and e[1] <= cases.bar_cents and e[2] <= cases.bar_db):
            bad.append((i, e))
        for f in np.nonzero(cases.lag_open[i])[0]:
            if not R.admissible(f0_raw, raw, f, t, cases.guard, cases.bar_per, cases.bar_cents):
                bad.append((i, int(f), "not an admissible answer"))
    assert not bad, bad


def test_gate_and_voicing_follow_the_float64_decisions(cases, tracks):
    for i, ((f0, per, raw, loud), t) in enumerate(zip(tracks, cases.t64)):
        silent, voiced = loud < np.float32(R.SILENCE), ~np.isnan(f0)
        # what the kernel gives out is made of its own taps, on every frame
        assert np.array_equal(per, np.where(silent, np.float32(0), raw)) and np.array_equal(voiced, per >= np.float32(R.UNVOICED)), i
        sure = ~cases.open[i]
        assert np.array_equal(silent[sure], (t.loud < R.SILENCE)[sure]) and np.array_equal(voiced[sure], ~np.isnan(t.f0)[sure]), i
        cents = 1200.0 * np.log2(f0[sure & voiced].astype(np.float64) / t.f0[sure & voiced])
        assert float(np.abs(cents).max()) <= cases.bar_cents, i
        if i % (1 + len(R.SNRS)) == 0:                              # the clip itself (noise fills its twins' silence)
            assert 0.05 < silent.mean() < 0.3 and 0.5 < voiced.mean() < 0.85, i      # the recipe has silent, noisy and voiced frames


def test_pairs_against_float64(cases, tracks):
    got, intact = R.run_pairs([cases.signals[i] for i, _ in cases.pairs], [cases.signals[j] for _, j in cases.pairs])
    assert intact
    bad = []
    for (i, j), g in zip(cases.pairs, got):
        want = cases.pair_want(i, j, *(SimpleNamespace(f0=tracks[k][0], per=tracks[k][1]) for k in (i, j)))
        err, bar = R.metric_error(g, want), cases.pair_bar(want)
        print(f"pitch_pairs ({i}, {j})  got {g}  float64 {want}  error {err}  (bar {bar})")
        if not bool((err <= bar).all()):
            bad.append(((i, j), err, bar))
    assert not bad, bad
    f1, cents = np.array([g[2] for g in got]), np.array([g[1] for g in got])
    assert f1.min() < 0.97 and f1.max() == 1.0 and cents.min() < 1.0 and cents.max() > 100.0     # all three outputs move


EDGES = (1024, 1183, 1184, 1024 + 160 * 63 - 1, 1024 + 160 * 63, 1024 + 160 * 63 + 1)


def test_lengths_at_the_frame_edges(cases):
    """One frame, the last sample before a second one, two frames; 63, 64 and 64 frames: the last workgroup of four full or not."""
    x = cases.signals[0]
    clips = [x[2000:2000 + T] for T in EDGES]
    got, intact = R.run_track(clips)
    assert intact and [len(g[0]) for g in got] == [1, 1, 2, 63, 64, 64]
    for c, (f0, per, raw, loud) in zip(clips, got):
        t = R.Track(c)
        lag_open, gate_open, den_open = R.decisions(t, cases.guard, cases.guard_db)
        f0_raw = np.where(np.isnan(f0), t.f0_raw, f0)
        e = R.tap_errors(f0_raw, raw, loud, t, lag_open, den_open, cases.guard)
        assert e[0] <= cases.bar_per and e[1] <= cases.bar_cents and e[2] <= cases.bar_db, (len(c), e)
        sure = ~(lag_open | gate_open | den_open)
        assert np.array_equal(np.isnan(f0)[sure], np.isnan(t.f0)[sure]), len(c)
    # a frame's YIN values depend on its 1024 samples alone (the loudness does not: the floor is the clip's)
    assert np.array_equal(got[0][2], got[2][2][:1]) and np.array_equal(got[3][2], got[4][2][:63]) and np.array_equal(got[4][2], got[5][2])


def _mixed(n):
    """n short pairs of mixed lengths: pieces of the recipe clips and their noisy twins."""
    lengths = (1024, 1500, 2047, 4100, 1184)
    src, refs, ests = R.cases().signals, [], []
    for i in range(n):
        T, at = lengths[i % 5], 37 * i
        refs.append(src[4 * (i % 2)][at:at + T])
        ests.append(src[4 * (i % 2) + 1 + i % 3][at:at + T])
    return refs, ests


def test_bit_identity_alone_in_a_batch_on_both_routes_and_over_the_workspace(cases):
    """A pair alone; in calls of 2, 64 (descriptors in the argument block) and 65 pairs (descriptors through the workspace) of mixed
    lengths at the first, a middle and the last position, whatever the workspace held before; and the same for the tracks."""
    x, y = cases.signals[0][1000:6000], cases.signals[2][1000:6000]
    (alone,), ok = R.run_pairs([x], [y])
    assert ok and np.isfinite(alone).all()
    for n in (2, 64, 65):
        refs, ests = _mixed(n)
        others, ok = R.run_pairs(refs, ests)
        assert ok
        positions = sorted({0, n // 2, n - 1})
        for pos in positions:
            refs[pos], ests[pos] = x, y
        for fill in (0xAB, 0xFF, 0x00) if n == 65 else (0xAB,):
            got, ok = R.run_pairs(refs, ests, ws_fill=fill)
            assert ok
            for k in range(n):
                assert np.array_equal(got[k], alone if k in positions else others[k], equal_nan=True), (n, fill, k)
    (one,), ok = R.run_track([x])
    refs, _ = _mixed(69)
    many, ok2 = R.run_track(refs + [x], ws_fill=0xFF)                # 70 clips: through the workspace
    three, ok3 = R.run_track([refs[1], x, refs[2]], ws_fill=0x00, taps=False)
    assert ok and ok2 and ok3
    for k in range(4):
        assert np.array_equal(many[-1][k], one[k], equal_nan=True)
    assert np.array_equal(three[1][0], one[0], equal_nan=True) and np.array_equal(three[1][1], one[1]) and three[1][2] is None
    assert np.array_equal(three[0][1], many[1][1]) and np.array_equal(three[2][0], many[2][0], equal_nan=True)


@pytest.mark.parametrize("freq", [50.5, 60.0, 100.0, 440.0, 530.0, 1000.0])
def test_pure_tones(freq):
    """The tones of tests/test_pitch_host.py: within 1.5 cents with periodicity > 0.999, 1000 Hz as its 500 Hz subharmonic."""
    ((f0, per, raw, loud),), ok = R.run_track([R.tone(freq)])
    want = freq if freq <= 550 else freq / 2
    cents = np.abs(1200.0 * np.log2(f0.astype(np.float64) / want))
    assert ok and len(f0) == 19 and float(cents.max()) < 1.5 and float(raw.min()) > 0.999 and np.array_equal(per, raw), (cents.max(), raw.min())


def test_digital_silence_and_dc():
    z, dc = np.zeros(4000, np.float32), np.full(4000, 0.25, np.float32)
    got, ok = R.run_track([z, dc])
    assert ok
    for f0, per, raw, loud in got:
        assert bool((raw == 0).all()) and bool((per == 0).all()) and np.isnan(f0).all()
    assert bool((got[0][3] < -100).all())
    pairs, ok = R.run_pairs([z, dc, z], [z, dc, R.tone(100.0)])
    assert ok
    for g in pairs[:2]:
        assert g[0] == 0 and np.isnan(g[1]) and np.isnan(g[2])
    assert pairs[2][0] > 0.99 and np.isnan(pairs[2][1]) and np.isnan(pairs[2][2])     # nothing voiced in the reference: recall is 0 / 0


def test_gain_by_a_power_of_two_moves_no_bit_of_the_yin_taps(cases):
    """d scales by the gain's square exactly, so d', the lag, the pitch and the ungated periodicity keep every bit.  The gate moves
    with the gain, by definition: the pitch is read from a call in which no frame is silent or unvoiced."""
    x = cases.signals[0]
    got, ok = R.run_track([x, (x * np.float32(4)), (x * np.float32(0.125))], silence=-1e30, unvoiced=-1.0)
    assert ok and not np.isnan(got[0][0]).any()
    for g in got[1:]:
        assert np.array_equal(g[2], got[0][2]) and np.array_equal(g[0], got[0][0])
    assert float(np.abs(got[1][3] - got[0][3] - 20 * np.log10(4.0)).max()) < 1e-3    # the loudness moves by the gain, floor included
    gated, ok = R.run_track([x, (x * np.float32(0.125))])
    assert ok and (gated[1][1] == 0).sum() > (gated[0][1] == 0).sum()                # 18 dB down: more frames are silent
