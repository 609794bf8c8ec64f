"""Pitch, periodicity and the voiced / unvoiced F1 of csrc/pitch.hip (include/wavtokenizer_amd.h gives the definition) in float64
numpy, written from that definition: the frame grid, the loudness gate and the three formulas of the reference's
metrics/periodicity.py, with YIN (de Cheveigne & Kawahara 2002) where the reference runs CREPE.  The same code runs in fp32 as the
stand-in that sets the tests' error bars (dtype=np.float32: every difference, product and sum rounded to fp32, the difference
function added term by term, the transform by torch.fft.rfft on fp32 on the CPU), and the module holds the decision margins, the
test signals and the ctypes plumbing the tests share."""
import functools

import numpy as np

from tests.mel_ref import Arena, Outputs

RATE, WIN, HOP = 16000, 1024, 160
MAX_LAG, TERMS = 321, 703
LAG_LO, LAG_HI = 30, 320
BINS = WIN // 2 + 1
THRESHOLD, SILENCE, UNVOICED = 0.15, -60.0, 0.5


def n_frames(T: int) -> int:
    return 0 if T < WIN else 1 + (T - WIN) // HOP


def window64():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN, dtype=np.float64) / WIN)


def a_weighting64():
    """librosa.A_weighting(librosa.fft_frequencies(sr=16000, n_fft=1024)) in float64: clipped below at -80 dB, bin 0 gets -80."""
    f = np.arange(BINS, dtype=np.float64) * RATE / WIN
    c = np.array([12194.217, 20.598997, 107.65265, 737.86223]) ** 2
    q = f ** 2
    with np.errstate(divide="ignore"):
        w = 2.0 + 20.0 * (np.log10(c[0]) + 2.0 * np.log10(q) - np.log10(q + c[0]) - np.log10(q + c[1]) - 0.5 * np.log10(q + c[2])
                          - 0.5 * np.log10(q + c[3]))
    return np.maximum(w, -80.0)


def frames(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    n = n_frames(x.shape[0])
    assert x.ndim == 1 and n >= 1
    return x[np.arange(n)[:, None] * HOP + np.arange(WIN)[None, :]]


def cmnd(fr, dtype=np.float64):
    """d' [F][322] (column 0 unused, 1.0): the difference function over 703 terms per lag, added term by term (fp32: in that order,
    one rounding per term), and its cumulative-mean normalisation; 1 where the running sum is 0."""
    F = fr.shape[0]
    d = np.zeros((F, MAX_LAG + 1), dtype)
    for lag in range(1, MAX_LAG + 1):
        e = fr[:, :TERMS] - fr[:, lag:lag + TERMS]
        sq = (e * e).astype(dtype)
        d[:, lag] = sq.sum(axis=1) if dtype == np.float64 else np.cumsum(sq, axis=1, dtype=dtype)[:, -1]
    run = np.cumsum(d[:, 1:], axis=1, dtype=dtype)
    dp = np.ones((F, MAX_LAG + 1), dtype)
    lags = np.arange(1, MAX_LAG + 1).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        dp[:, 1:] = np.where(run > 0, (d[:, 1:] * lags[None, :]).astype(dtype) / run, dtype(1))
    return dp


def pick(dp, threshold=THRESHOLD):
    """Per frame the lag: the first in [30, 320] under the threshold that is a local minimum (<= left, < right), else the smallest
    lag that attains the minimum over the range."""
    cur, le, ri = dp[:, LAG_LO:LAG_HI + 1], dp[:, LAG_LO - 1:LAG_HI], dp[:, LAG_LO + 1:LAG_HI + 2]
    ok = (cur < threshold) & (cur <= le) & (cur < ri)
    return LAG_LO + np.where(ok.any(axis=1), ok.argmax(axis=1), cur.argmin(axis=1))


def refine(dp, lag, dtype=np.float64):
    """(f0, periodicity) of the parabola through d' at lag - 1, lag, lag + 1."""
    i = np.arange(dp.shape[0])
    a, b, c = dp[i, lag - 1], dp[i, lag], dp[i, lag + 1]
    den = (a - dtype(2) * b + c).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        off = np.where(den > 0, np.clip((dtype(0.5) * (a - c)).astype(dtype) / den, -0.5, 0.5), 0).astype(dtype)
    f0 = (dtype(RATE) / (lag.astype(dtype) + off)).astype(dtype)
    per = np.clip(dtype(1) - (b - (dtype(0.25) * (a - c)).astype(dtype) * off), 0, 1).astype(dtype)
    return f0, per


def loudness(fr, dtype=np.float64):
    """Per frame the mean over the 513 bins of max(10 log10 max(S, 1e-10), clip maximum - 80) + A - 20."""
    if dtype == np.float64:
        X = np.fft.rfft(fr * window64()[None, :], axis=1)
        S = X.real ** 2 + X.imag ** 2
    else:
        import torch
        X = torch.fft.rfft(torch.from_numpy((fr * window64().astype(dtype)[None, :]).astype(dtype)), dim=1)
        S = (X.real ** 2 + X.imag ** 2).numpy().astype(dtype)
    db = (dtype(10) * np.log10(np.maximum(S, dtype(1e-10)))).astype(dtype)
    db = np.maximum(db, db.max() - dtype(80))
    lv = ((db + a_weighting64().astype(dtype)[None, :]).astype(dtype) - dtype(20)).astype(dtype)
    return lv.mean(axis=1, dtype=dtype)


def gate(f0, per_raw, loud, silence=SILENCE, unvoiced=UNVOICED):
    """(f0 with NaN on unvoiced frames, gated periodicity)."""
    per = np.where(loud < silence, 0, per_raw).astype(per_raw.dtype)
    return np.where(per < unvoiced, np.nan, f0).astype(f0.dtype), per


class Track:
    """Everything about one clip at one precision: dp, lag, f0_raw, per_raw, loud, f0 (NaN: unvoiced), per."""

    def __init__(self, x, dtype=np.float64, threshold=THRESHOLD, silence=SILENCE, unvoiced=UNVOICED):
        fr = frames(x, dtype)
        self.dp = cmnd(fr, dtype)
        self.lag = pick(self.dp, dtype(threshold))
        self.f0_raw, self.per_raw = refine(self.dp, self.lag, dtype)
        self.loud = loudness(fr, dtype)
        self.f0, self.per = gate(self.f0_raw, self.per_raw, self.loud, dtype(silence), dtype(unvoiced))
        self.n = fr.shape[0]


def pair_metrics(f0, per, f0_hat, per_hat, dtype=np.float64):
    """(periodicity_loss, pitch_loss, f1) of calculate_periodicity_metrics on two tracks (reference first); NaN as numpy gives it.
    dtype=np.float32: every step rounded to fp32, the stand-in of the pair reduction."""
    f0, per, f0_hat, per_hat = (np.asarray(v, dtype) for v in (f0, per, f0_hat, per_hat))
    tv, pv = ~np.isnan(f0), ~np.isnan(f0_hat)
    both = tv & pv
    with np.errstate(divide="ignore", invalid="ignore"):
        ploss = np.sqrt((((per_hat - per) ** 2).astype(dtype).sum(dtype=dtype) / dtype(len(per))).astype(dtype))
        cents = (dtype(1200) * (np.log2(f0[both]) - np.log2(f0_hat[both])).astype(dtype)).astype(dtype)
        pitch = np.sqrt(((cents ** 2).astype(dtype).sum(dtype=dtype) / dtype(both.sum())).astype(dtype))
        tp, fp, fn = dtype(both.sum()), dtype((~tv & pv).sum()), dtype((tv & ~pv).sum())
        precision, recall = tp / (tp + fp), tp / (tp + fn)
        f1 = dtype(2) * precision * recall / (precision + recall)
    return np.array([ploss, pitch, f1], np.float64)


def periodicity_metrics64(y, y_hat, **kw):
    a, b = Track(y, **kw), Track(y_hat, **kw)
    return pair_metrics(a.f0, a.per, b.f0, b.per)


# ------------------------------------------------------------------------------------------------ decisions and errors
def admissible_lags(dp_row, guard, threshold=THRESHOLD):
    """The lags a frame may come out with when every comparison of the search is allowed to fall either way inside guard."""
    lags = np.arange(LAG_LO, LAG_HI + 1)
    cur, le, ri = dp_row[lags], dp_row[lags - 1], dp_row[lags + 1]
    ok = (cur < threshold + guard) & (cur <= le + guard) & (cur < ri + guard)
    sure = (cur < threshold - guard) & (cur <= le - guard) & (cur < ri - guard)
    if sure.any():                                                  # nothing behind the first certain candidate can be picked
        ok[sure.argmax() + 1:] = False
        return lags[ok]
    return lags[ok | (cur <= cur.min() + guard)]


def decisions(t: "Track", guard, guard_db, threshold=THRESHOLD, silence=SILENCE, unvoiced=UNVOICED):
    """Per frame of a float64 track: (lag_open, gate_open).  lag_open: more than one admissible lag inside guard (d' against the
    threshold or a neighbour at a lag the search reaches, or a tie of the fallback minimum).  gate_open: the periodicity within
    guard of unvoiced_threshold (for any admissible lag) or the loudness within guard_db of silence_threshold."""
    lag_open, gate_open = np.zeros(t.n, bool), np.zeros(t.n, bool)
    for f in range(t.n):
        adm = admissible_lags(t.dp[f], guard, threshold)
        lag_open[f] = len(adm) != 1 or adm[0] != t.lag[f]
        pers = refine(np.repeat(t.dp[f][None, :], len(adm), 0), adm)[1] if lag_open[f] else t.per_raw[f:f + 1]
        gate_open[f] = bool((np.abs(pers - unvoiced) <= guard).any()) or abs(t.loud[f] - silence) <= guard_db
    return lag_open, gate_open


def tap_errors(got_f0, got_per, got_loud, t: "Track", lag_open):
    """(periodicity error, cents error, loudness error in dB): the largest over the frames; a frame with an open lag decision is
    held against the admissible answer nearest to what it gave (per and cents), and every frame counts for the loudness."""
    e_per, e_cents = 0.0, 0.0
    for f in range(t.n):
        if lag_open[f]:
            lags = np.arange(LAG_LO, LAG_HI + 1)
            f0s, pers = refine(np.repeat(t.dp[f][None, :], len(lags), 0), lags)
            k = int(np.abs(1200.0 * np.log2(float(got_f0[f]) / f0s)).argmin())
            f0, per = f0s[k], pers[k]
        else:
            f0, per = t.f0_raw[f], t.per_raw[f]
        e_per = max(e_per, abs(float(got_per[f]) - per))
        e_cents = max(e_cents, abs(1200.0 * np.log2(float(got_f0[f]) / f0)))
    return e_per, e_cents, float(np.abs(np.asarray(got_loud, np.float64) - t.loud).max())


def admissible(got_f0, got_per_raw, f, t: "Track", guard, bar_per, bar_cents, threshold=THRESHOLD):
    """Whether frame f's (f0, ungated periodicity) is one of the answers its admissible lags give in float64, within the bars."""
    adm = admissible_lags(t.dp[f], guard, threshold)
    f0s, pers = refine(np.repeat(t.dp[f][None, :], len(adm), 0), adm)
    return bool(((np.abs(1200.0 * np.log2(float(got_f0[f]) / f0s)) <= bar_cents) & (np.abs(float(got_per_raw[f]) - pers) <= bar_per)).any())


def with_decisions_of(t: "Track", got_f0, got_per, open_frames):
    """The float64 gated tracks with the frames in open_frames replaced by what the code under test decided there."""
    f0, per = t.f0.copy(), t.per.copy()
    f0[open_frames] = np.asarray(got_f0, np.float64)[open_frames]
    per[open_frames] = np.asarray(got_per, np.float64)[open_frames]
    return f0, per


def metric_error(got, want):
    """The largest |got - want| over the three pair metrics; NaN must meet NaN (inf otherwise)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return np.full(3, np.inf)
    return np.where(np.isnan(want), 0.0, np.abs(got - want))


# ------------------------------------------------------------------------------------------------ signals
def tone(freq, T=4000, amp=0.5, seed=0):
    """A pure tone with a noise floor 50 dB under it."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64) / RATE
    x = amp * np.sin(2 * np.pi * freq * t)
    return (x + amp / np.sqrt(2) * 10 ** (-50 / 20) * rng.standard_normal(T)).astype(np.float32)


def recipe(T, seed):
    """A harmonic source of 8 partials (f0 drawn from 80..400 Hz, 3 % vibrato at 5 Hz) over a 2e-3 white noise floor, one sixth of
    the clip replaced by white noise at 0.05 and one sixth by near-silence at 1e-5."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64) / RATE
    f0 = rng.uniform(80.0, 400.0)
    phase = 2 * np.pi * np.cumsum(f0 * (1.0 + 0.03 * np.sin(2 * np.pi * 5.0 * t))) / RATE
    x = sum(0.3 / k * np.sin(k * phase + rng.uniform(0, 2 * np.pi)) for k in range(1, 9))
    x = x + 2e-3 * rng.standard_normal(T)
    sixth = T // 6
    a, b = sorted(rng.choice(5, 2, replace=False))
    x[a * sixth:(a + 1) * sixth] = 0.05 * rng.standard_normal(sixth)
    x[b * sixth + sixth // 2:(b + 1) * sixth + sixth // 2] = 1e-5 * rng.standard_normal(sixth)
    return x.astype(np.float32)


def decoded(x, snr_db, seed):
    """The clip plus white noise at snr_db."""
    rng = np.random.default_rng(9000 + seed)
    p = float(np.mean(np.asarray(x, np.float64) ** 2))
    return (x + np.sqrt(p / 10 ** (snr_db / 10)) * rng.standard_normal(len(x))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the calls, through ctypes
@functools.lru_cache(maxsize=None)
def handle():
    from wavtokenizer_amd import metrics
    return metrics.pitch_handle(0)


def _workspace(n, total, ws_fill):
    import torch

    from wavtokenizer_amd._capi import lib
    nbytes = int(lib.wt_pitch_workspace_bytes(n, total))
    return torch.full((nbytes + 64,), ws_fill, dtype=torch.uint8, device="cuda"), nbytes


def run_track(clips, threshold=THRESHOLD, silence=SILENCE, unvoiced=UNVOICED, ws_fill=0xAB, taps=True):
    """One wt_pitch_track call on clips laid out in a NaN arena, outputs and taps between canaries, the workspace filled with ws_fill
    beforehand.  ([(f0, periodicity, raw periodicity, loudness)] per clip, canaries intact)."""
    import ctypes

    import torch

    from wavtokenizer_amd._capi import WtPitchClip, check, lib
    n = len(clips)
    arena = Arena(list(clips))
    F = [n_frames(len(c)) for c in clips]
    outs = Outputs([2 * f for f in F] * (2 if taps else 1))
    ws, nbytes = _workspace(n, sum(F), ws_fill)
    descs = (WtPitchClip * n)()
    for i in range(n):
        descs[i].signal, descs[i].length, descs[i].out = arena.ptr(i), len(clips[i]), outs.ptr(i)
        descs[i].taps = outs.ptr(n + i) if taps else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.wt_pitch_track(handle(), descs, n, threshold, silence, unvoiced, ctypes.c_void_p(ws.data_ptr()), stream), "wt_pitch_track")
    torch.cuda.synchronize()
    got, intact = outs.read()
    assert bool((ws[nbytes:] == ws_fill).all()), "the call wrote behind its workspace"
    if not taps:
        return [(got[i][:F[i]], got[i][F[i]:], None, None) for i in range(n)], intact
    return [(got[i][:F[i]], got[i][F[i]:], got[n + i][:F[i]], got[n + i][F[i]:]) for i in range(n)], intact


def run_pairs(refs, ests, threshold=THRESHOLD, silence=SILENCE, unvoiced=UNVOICED, ws_fill=0xAB):
    """One wt_pitch_pairs call on pairs laid out in a NaN arena, outputs between canaries.  ([3] float32 arrays, canaries intact)."""
    import ctypes

    import torch

    from wavtokenizer_amd._capi import WtPitchPair, check, lib
    n = len(refs)
    arena = Arena(list(refs) + list(ests))
    outs = Outputs([3] * n)
    ws, nbytes = _workspace(n, sum(n_frames(len(c)) for c in refs), ws_fill)
    descs = (WtPitchPair * n)()
    for i in range(n):
        descs[i].reference, descs[i].estimate, descs[i].length, descs[i].out = arena.ptr(i), arena.ptr(n + i), len(refs[i]), outs.ptr(i)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.wt_pitch_pairs(handle(), descs, n, threshold, silence, unvoiced, ctypes.c_void_p(ws.data_ptr()), stream), "wt_pitch_pairs")
    torch.cuda.synchronize()
    got, intact = outs.read()
    assert bool((ws[nbytes:] == ws_fill).all()), "the call wrote behind its workspace"
    return got, intact


# ------------------------------------------------------------------------------------------------ the cases the GPU tests share
CLIPS = ((16000, 0), (24037, 1))                # (samples, seed) of recipe(); each with its decoded twins at SNRS
SNRS = (30, 10, 0)
BAR_FACTOR, GUARD_FACTOR, OPEN_CAP = 4.0, 10.0, 0.02


class Cases:
    """The test signals with their float64 tracks, computed once: the bars of the three taps (BAR_FACTOR x what the fp32 stand-in
    reaches on these signals against float64), the guards (GUARD_FACTOR x the bars), the frames whose decisions lie inside them,
    and the pairs (clip, twin) with the stand-in's pair error."""

    def __init__(self, clips=CLIPS, snrs=SNRS):
        self.signals, self.pairs = [], []
        for T, seed in clips:
            x = recipe(T, seed)
            self.signals.append(x)
            for snr in snrs:
                self.pairs.append((len(self.signals) - 1 - snrs.index(snr), len(self.signals)))
                self.signals.append(decoded(x, snr, seed))
        self.t64 = [Track(x) for x in self.signals]
        self.t32 = [Track(x, np.float32) for x in self.signals]
        # the stand-in's errors, a frame where it found another lag held against the nearest answer
        flipped = [a.lag != b.lag for a, b in zip(self.t64, self.t32)]
        worst = np.max([tap_errors(s.f0_raw, s.per_raw, s.loud, t, fl) for t, s, fl in zip(self.t64, self.t32, flipped)], axis=0)
        self.standin = tuple(float(v) for v in worst)
        self.bar_per, self.bar_cents, self.bar_db = (BAR_FACTOR * v for v in self.standin)
        self.guard, self.guard_db = GUARD_FACTOR * self.bar_per, GUARD_FACTOR * self.bar_db
        opened = [decisions(t, self.guard, self.guard_db) for t in self.t64]
        self.lag_open, self.gate_open = [o[0] for o in opened], [o[1] for o in opened]
        self.open = [a | b for a, b in opened]
        self.standin_flips_covered = all(bool((lo | ~fl).all()) for lo, fl in zip(self.lag_open, flipped))
        self.open_fraction = [float(o.mean()) for o in self.open]
        # the stand-in's pair error: its fp32 reduction of its own tracks against float64 on its decisions at the open frames
        self.standin_pair = np.zeros(3)
        for i, j in self.pairs:
            got = pair_metrics(self.t32[i].f0, self.t32[i].per, self.t32[j].f0, self.t32[j].per, np.float32)
            self.standin_pair = np.maximum(self.standin_pair, metric_error(got, self.pair_want(i, j, self.t32[i], self.t32[j])))

    def pair_want(self, i, j, a, b):
        """Float64 pair metrics of signals (i, j) with the decisions of the tracks a, b (objects with f0 and per) at the open frames."""
        f0, per = with_decisions_of(self.t64[i], a.f0, a.per, self.open[i])
        g0, qer = with_decisions_of(self.t64[j], b.f0, b.per, self.open[j])
        return pair_metrics(f0, per, g0, qer)

    def pair_bar(self, want):
        """BAR_FACTOR x the stand-in's pair error, and never under BAR_FACTOR half-units of fp32 at the value: the result is an fp32."""
        want = np.where(np.isnan(want), 0.0, np.abs(want))
        return BAR_FACTOR * np.maximum(self.standin_pair, 2.0 ** -24 * want)


@functools.lru_cache(maxsize=None)
def cases():
    return Cases()
