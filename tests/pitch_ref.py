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


def candidates(dp, threshold=THRESHOLD):
    """[F][291]: the lags in [30, 320] under the threshold that are a local minimum (<= left, < right)."""
    cur, le, ri = dp[:, LAG_LO:LAG_HI + 1], dp[:, LAG_LO - 1:LAG_HI], dp[:, LAG_LO + 1:LAG_HI + 2]
    return (cur < threshold) & (cur <= le) & (cur < ri)


def pick(dp, threshold=THRESHOLD):
    """Per frame the lag: the first in [30, 320] under the threshold that is a local minimum (<= left, < right), else the smallest
    lag that attains the minimum over the range."""
    ok = candidates(dp, threshold)
    return LAG_LO + np.where(ok.any(axis=1), ok.argmax(axis=1), dp[:, LAG_LO:LAG_HI + 1].argmin(axis=1))


def parabola(dp, lag, dtype=np.float64):
    """(a, b, c, den, off) of the parabola through d' at lag - 1, lag, lag + 1: off = 0 where den = a - 2 b + c is not positive."""
    i = np.arange(dp.shape[0])
    a, b, c = dp[i, lag - 1], dp[i, lag], dp[i, lag + 1]
    den = (a - dtype(2) * b + c).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        off = np.where(den > 0, np.clip((dtype(0.5) * (a - c)).astype(dtype) / den, -0.5, 0.5), 0).astype(dtype)
    return a, b, c, den, off


def from_offset(lag, a, b, c, off, dtype=np.float64):
    """(f0, periodicity) of a lag and an offset on its parabola."""
    f0 = (dtype(RATE) / (np.asarray(lag).astype(dtype) + off)).astype(dtype)
    per = np.clip(dtype(1) - (b - (dtype(0.25) * (a - c)).astype(dtype) * off), 0, 1).astype(dtype)
    return f0, per


def refine(dp, lag, dtype=np.float64):
    """(f0, periodicity) of the parabola through d' at lag - 1, lag, lag + 1."""
    a, b, c, _, off = parabola(dp, lag, dtype)
    return from_offset(lag, a, b, c, off, dtype)


def loudness(fr, dtype=np.float64, one_frame_clips=False):
    """Per frame the mean over the 513 bins of max(10 log10 max(S, 1e-10), clip maximum - 80) + A - 20; with one_frame_clips every
    row of fr is a clip of its own, and the maximum is the row's."""
    if dtype == np.float64:
        X = np.fft.rfft(fr * window64()[None, :], axis=1)
        S = X.real ** 2 + X.imag ** 2
    else:
        import torch
        X = torch.fft.rfft(torch.from_numpy((fr * window64().astype(dtype)[None, :]).astype(dtype)), dim=1)
        S = (X.real ** 2 + X.imag ** 2).numpy().astype(dtype)
    db = (dtype(10) * np.log10(np.maximum(S, dtype(1e-10)))).astype(dtype)
    db = np.maximum(db, (db.max(axis=1, keepdims=True) if one_frame_clips else db.max()) - dtype(80))
    lv = ((db + a_weighting64().astype(dtype)[None, :]).astype(dtype) - dtype(20)).astype(dtype)
    return lv.mean(axis=1, dtype=dtype)


def gate(f0, per_raw, loud, silence=SILENCE, unvoiced=UNVOICED):
    """(f0 with NaN on unvoiced frames, gated periodicity)."""
    per = np.where(loud < silence, 0, per_raw).astype(per_raw.dtype)
    return np.where(per < unvoiced, np.nan, f0).astype(f0.dtype), per


class Track:
    """Everything about one clip at one precision: dp, lag, f0_raw, per_raw, loud, f0 (NaN: unvoiced), per.  With one_frame_clips x is
    [N][1024]: N clips of one frame each, kept as the N frames of one track (the loudness floor is each clip's own).  d' and the
    loudness do not depend on the thresholds: at() gives the track at other thresholds without computing them again."""

    def __init__(self, x, dtype=np.float64, threshold=THRESHOLD, silence=SILENCE, unvoiced=UNVOICED, one_frame_clips=False):
        if isinstance(x, Track):
            dtype, self.dp, self.loud = x.dtype, x.dp, x.loud
        elif isinstance(x, tuple):                                  # (dtype, d', loudness) of some frames of another track
            dtype, self.dp, self.loud = x
        else:
            fr = np.asarray(x, dtype) if one_frame_clips else frames(x, dtype)
            assert fr.ndim == 2 and fr.shape[1] == WIN
            self.dp = cmnd(fr, dtype)
            self.loud = loudness(fr, dtype, one_frame_clips)
        self.dtype, self.n, self.setting = dtype, self.dp.shape[0], (threshold, silence, unvoiced)
        self.lag = pick(self.dp, dtype(threshold))
        self.f0_raw, self.per_raw = refine(self.dp, self.lag, dtype)
        _, _, _, self.den, self.off = parabola(self.dp, self.lag, dtype)
        self.f0, self.per = gate(self.f0_raw, self.per_raw, self.loud, dtype(silence), dtype(unvoiced))
        self.fallback = ~candidates(self.dp, dtype(threshold)).any(axis=1)        # no candidate: the minimum over the range

    def at(self, threshold=THRESHOLD, silence=SILENCE, unvoiced=UNVOICED):
        return Track(self, threshold=threshold, silence=silence, unvoiced=unvoiced)

    def take(self, keep):
        """The track of the frames keep alone (for a track of one-frame clips: of those clips), at the same thresholds."""
        return Track((self.dtype, self.dp[keep], self.loud[keep]), self.dtype, *self.setting)


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


DEN_GUARDS = 4.0                                # |den| and |a - c| are sums of three and two d' values: their guard is 4 x d's


def answers(dp_row, lags, guard=None, got_f0=None):
    """(f0, periodicity) arrays: the float64 answers of a frame at the given lags.  With a guard, a lag whose |den| = |a - 2 b + c|
    lies within DEN_GUARDS x guard also gives the answers of off = 0 and off = 0.5 sign(a - c) (den may come out on either side of
    0, and a tiny positive den drives the offset into its clamp), and, where |a - c| lies within DEN_GUARDS x guard as well, of the
    offset in [-0.5, 0.5] nearest to the one got_f0 has at that lag (the quotient of two open numbers).  Pitch and periodicity of
    one answer come from one offset."""
    lags = np.asarray(lags)
    dp = np.repeat(dp_row[None, :], len(lags), 0)
    a, b, c, den, off = parabola(dp, lags)
    sel, offs = [np.arange(len(lags))], [off]
    if guard is not None:
        o = np.nonzero(np.abs(den) <= DEN_GUARDS * guard)[0]
        sel += [o, o]
        offs += [np.zeros(len(o)), 0.5 * np.sign(a - c)[o]]
        free = o[np.abs(a - c)[o] <= DEN_GUARDS * guard]
        if got_f0 is not None and len(free):
            sel.append(free)
            offs.append(np.clip(RATE / float(got_f0) - lags[free], -0.5, 0.5))
    sel, offs = np.concatenate(sel), np.concatenate(offs)
    return from_offset(lags[sel], a[sel], b[sel], c[sel], offs)


def decisions(t: "Track", guard, guard_db, threshold=THRESHOLD, silence=SILENCE, unvoiced=UNVOICED):
    """Per frame of a float64 track: (lag_open, gate_open, den_open).  lag_open: more than one admissible lag inside guard (d' against
    the threshold or a neighbour at a lag the search reaches, or a tie of the fallback minimum).  den_open: |den| of the parabola
    within DEN_GUARDS x guard at an admissible lag (its sign decides between off = 0 and the quotient).  gate_open: the periodicity
    of an admissible answer within guard of unvoiced_threshold or the loudness within guard_db of silence_threshold."""
    lag_open, gate_open, den_open = np.zeros(t.n, bool), np.zeros(t.n, bool), np.zeros(t.n, bool)
    for f in range(t.n):
        adm = admissible_lags(t.dp[f], guard, threshold)
        lag_open[f] = len(adm) != 1 or adm[0] != t.lag[f]
        den = t.dp[f][adm - 1] - 2.0 * t.dp[f][adm] + t.dp[f][adm + 1]
        den_open[f] = bool((np.abs(den) <= DEN_GUARDS * guard).any())
        pers = answers(t.dp[f], adm, guard)[1]
        if den_open[f]:                                             # (a free offset: the periodicity is linear in it, the ends bound it)
            a, b, c = t.dp[f][adm - 1], t.dp[f][adm], t.dp[f][adm + 1]
            pers = np.concatenate([pers] + [from_offset(adm, a, b, c, np.full(len(adm), o))[1] for o in (-0.5, 0.5)])
        gate_open[f] = bool((np.abs(pers - unvoiced) <= guard).any()) or abs(t.loud[f] - silence) <= guard_db
    return lag_open, gate_open, den_open


def frame_errors(got_f0, got_per, got_loud, t: "Track", lag_open, den_open=None, guard=None):
    """Per frame ([3][F]: periodicity error, cents error, loudness error in dB) and the float64 values they were taken against
    ([3][F]: periodicity, f0, loudness).  A frame with an open lag decision is held against the answer, of any lag, nearest to
    what it gave (per and cents), one with an open den decision (den_open and its guard given) against the nearest of answers() at
    its lag."""
    want = np.stack([t.per_raw, t.f0_raw, t.loud]).astype(np.float64)
    for f in range(t.n):
        if lag_open[f] or (den_open is not None and den_open[f]):
            lags = np.arange(LAG_LO, LAG_HI + 1) if lag_open[f] else t.lag[f:f + 1]
            f0s, pers = answers(t.dp[f], lags, guard if den_open is not None else None, got_f0[f])
            k = int(np.abs(1200.0 * np.log2(float(got_f0[f]) / f0s)).argmin())
            want[0, f], want[1, f] = pers[k], f0s[k]
    got_f0, got_per, got_loud = (np.asarray(v, np.float64) for v in (got_f0, got_per, got_loud))
    return np.stack([np.abs(got_per - want[0]), np.abs(1200.0 * np.log2(got_f0 / want[1])), np.abs(got_loud - want[2])]), want


def tap_errors(got_f0, got_per, got_loud, t: "Track", lag_open, den_open=None, guard=None):
    """(periodicity error, cents error, loudness error in dB): the largest of frame_errors() over the frames."""
    return tuple(float(v) for v in frame_errors(got_f0, got_per, got_loud, t, lag_open, den_open, guard)[0].max(axis=1))


def admissible(got_f0, got_per_raw, f, t: "Track", guard, bar_per, bar_cents, threshold=THRESHOLD):
    """Whether frame f's (f0, ungated periodicity) is one of the answers its admissible lags give in float64, within the bars."""
    adm = admissible_lags(t.dp[f], guard, threshold)
    f0s, pers = answers(t.dp[f], adm, guard, got_f0[f])
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
    and the pairs (clip, twin) with the stand-in's pair error.
    With base (the cases at the default thresholds) and setting = (threshold, silence, unvoiced): the same signals at that setting.
    d' and the loudness are the base's, as are the guards (the error of d' and of the loudness does not depend on a threshold);
    the lags, the parabolas, the gates, the decisions, the stand-in's errors and with them the bars are the setting's own."""

    def __init__(self, clips=CLIPS, snrs=SNRS, setting=(THRESHOLD, SILENCE, UNVOICED), base=None):
        self.setting = tuple(setting)
        if base is None:
            self.signals, self.pairs = [], []
            for T, seed in clips:
                x = recipe(T, seed)
                self.signals.append(x)
                for snr in snrs:
                    self.pairs.append((len(self.signals) - 1 - snrs.index(snr), len(self.signals)))
                    self.signals.append(decoded(x, snr, seed))
            self.t64 = [Track(x, np.float64, *setting) for x in self.signals]
            self.t32 = [Track(x, np.float32, *setting) for x in self.signals]
        else:
            self.signals, self.pairs = base.signals, base.pairs
            self.t64, self.t32 = [t.at(*setting) for t in base.t64], [t.at(*setting) for t in base.t32]
            self.guard, self.guard_db = base.guard, base.guard_db
            opened = [decisions(t, self.guard, self.guard_db, *setting) for t in self.t64]
        # the stand-in's errors, a frame where it found another lag held against the nearest answer (and at a setting of its own,
        # where the guards are known beforehand, a frame with an open den against the nearest of its answers)
        flipped = [a.lag != b.lag for a, b in zip(self.t64, self.t32)]
        den = [None] * len(flipped) if base is None else [o[2] for o in opened]
        worst = np.max([tap_errors(s.f0_raw, s.per_raw, s.loud, t, fl, d, None if base is None else self.guard)
                        for t, s, fl, d in zip(self.t64, self.t32, flipped, den)], axis=0)
        self.standin = tuple(float(v) for v in worst)
        self.bar_per, self.bar_cents, self.bar_db = (BAR_FACTOR * v for v in self.standin)
        if base is None:
            self.guard, self.guard_db = GUARD_FACTOR * self.bar_per, GUARD_FACTOR * self.bar_db
            opened = [decisions(t, self.guard, self.guard_db, *setting) for t in self.t64]
        self.lag_open, self.gate_open, self.den_open = ([o[k] for o in opened] for k in range(3))
        self.open = [a | b | c for a, b, c in opened]
        self.new_den_open = [int((c & ~(a | b)).sum()) for a, b, c in opened]    # frames that only the den decision opens
        self.standin_flips_covered = all(bool((lo | ~fl).all()) for lo, fl in zip(self.lag_open, flipped))
        self.open_fraction = [float(o.mean()) for o in self.open]
        # the stand-in's pair error: its fp32 reduction of its own tracks against float64 on its decisions at the open frames
        self.standin_pair, self.base_standin_pair = np.zeros(3), (np.zeros(3) if base is None else base.standin_pair)
        for i, j in self.pairs:
            got = pair_metrics(self.t32[i].f0, self.t32[i].per, self.t32[j].f0, self.t32[j].per, np.float32)
            self.standin_pair = np.maximum(self.standin_pair, metric_error(got, self.pair_want(i, j, self.t32[i], self.t32[j])))

    def pair_want(self, i, j, a, b):
        """Float64 pair metrics of signals (i, j) with the decisions of the tracks a, b (objects with f0 and per) at the open frames."""
        f0, per = with_decisions_of(self.t64[i], a.f0, a.per, self.open[i])
        g0, qer = with_decisions_of(self.t64[j], b.f0, b.per, self.open[j])
        return pair_metrics(f0, per, g0, qer)

    def pair_bar(self, want):
        """BAR_FACTOR x the stand-in's pair error, and never under BAR_FACTOR half-units of fp32 at the value: the result is an fp32.
        At a setting of its own the stand-in's pair error is the larger of the setting's and the default thresholds': the error
        of an fp32 reduction over the same six pairs does not depend on a threshold, each figure is the largest of six samples
        of it (3.6e-5 .. 1.6e-4 cents over the grid where the taps err alike), and the default one is the yardstick these pairs
        have in tests/test_pitch_op.py; a setting whose taps err more (threshold 10: lag 30 in noise) adds its own."""
        want = np.where(np.isnan(want), 0.0, np.abs(want))
        return BAR_FACTOR * np.maximum(np.maximum(self.standin_pair, self.base_standin_pair), 2.0 ** -24 * want)


@functools.lru_cache(maxsize=None)
def cases():
    return Cases()


# (threshold, silence, unvoiced) of the threshold grid: the fallback on every frame and on none, thresholds around the default,
# and gates that silence most of a clip, voice everything and voice nothing
SETTINGS = ((0.0, -60.0, 0.5), (0.05, -60.0, 0.5), (0.3, -60.0, 0.5), (1.0, -60.0, 0.5), (10.0, -60.0, 0.5),
            (0.15, -40.0, 0.21), (0.15, -80.0, 0.9), (0.15, -50.0, 0.0), (0.15, -70.0, 1.0))


@functools.lru_cache(maxsize=None)
def cases_at(setting):
    return Cases(setting=setting, base=cases())


# ------------------------------------------------------------------------------------------------ every lag and the range's edges
EVERY = dict(silence=-1e30, unvoiced=-1.0)      # a call in which no frame is silent or unvoiced: f0 is the raw pitch of every frame


def edge_tone(period, seed, K, noise=2e-3, T=WIN):
    """K partials 0.3 / k of a tone with the given period in samples, phases drawn in order, over white noise."""
    rng = np.random.default_rng(seed)
    n = np.arange(T, dtype=np.float64)
    x = np.zeros(T)
    for k in range(1, K + 1):
        x += 0.3 / k * np.sin(2.0 * np.pi * k * n / period + rng.uniform(0, 2.0 * np.pi))
    return (x + noise * rng.standard_normal(T)).astype(np.float32)


# (period, seed, K).  The sweep: the .3 / .8 fractions keep d'(P) and d'(P +- 1) apart (at .0 / .5 nearly half of the frames tie);
# periods under 30 resolve to their subharmonic, periods past 320.5 to lag 320 with the offset in its clamp.  The pool of low tones
# (11.4 .. 49.8 Hz, under the search range): d' is nearly straight at lag 320 and den about 1e-6, of either sign.
SWEEP = tuple((28.8 + 0.5 * i, 100 + i, 3) for i in range(591))
LOW_POOL = tuple((float(p), 5000 + p, 1) for p in range(LAG_HI + 1, 1401))
HALF_UNIT = 2.0 ** -24                          # of fp32, relative: the least a bar may be is BAR_FACTOR of these at the value


class EdgeSet:
    """One-frame clips (edge_tone) as one track of N frames in float64 and in the fp32 stand-in, with the decisions under the
    recipe clips' guards in a call in which nothing is gated (EVERY).  sure_only keeps the clips whose frame is sure under every
    guard (the selection runs here, from the pool, every time) and remembers what the pool showed.  The bars are the set's own:
    BAR_FACTOR x the stand-in's error on the set, never under BAR_FACTOR half-units of fp32 at the value."""

    def __init__(self, tones, recipe: "Cases", sure_only=False):
        self.guard, self.guard_db = guard, guard_db = recipe.guard, recipe.guard_db
        self.signals = [edge_tone(*t) for t in tones]
        self.t64 = Track(np.stack(self.signals), one_frame_clips=True, **EVERY)
        self.t32 = Track(np.stack(self.signals), np.float32, one_frame_clips=True, **EVERY)
        self.lag_open, self.gate_open, self.den_open = decisions(self.t64, guard, guard_db, THRESHOLD, **EVERY)
        self.pool_n = len(tones)
        same = self.t32.lag == self.t64.lag
        self.pool_den_flips = same & ((self.t32.den > 0) != (self.t64.den > 0))      # the stand-in's den on the other side of 0
        self.pool_den_flips_covered = bool((self.den_open | ~self.pool_den_flips).all())
        self.pool_den_near = int((np.abs(self.t64.den) <= DEN_GUARDS * guard).sum())
        if sure_only:
            keep = np.nonzero(~(self.lag_open | self.gate_open | self.den_open))[0]
            self.signals = [self.signals[k] for k in keep]
            self.t64, self.t32 = self.t64.take(keep), self.t32.take(keep)
            self.lag_open, self.gate_open, self.den_open = self.lag_open[keep], self.gate_open[keep], self.den_open[keep]
        self.open = self.lag_open | self.gate_open | self.den_open
        self.sure = ~self.open
        self.flipped = self.t32.lag != self.t64.lag
        self.standin_flips_covered = bool((self.lag_open | ~self.flipped).all())
        err, _ = frame_errors(self.t32.f0_raw, self.t32.per_raw, self.t32.loud, self.t64, self.lag_open | self.flipped, self.den_open, guard)
        self.standin = tuple(float(v) for v in err.max(axis=1))
        # a set cannot buy itself a looser bar than the recipe clips': where its stand-in errs more, the recipe's error sets the bar
        # (the loudness does, by a percent or by a quarter from one CPU to the next: its stand-in is the platform's fp32 FFT, and
        # the largest of a few hundred frames' errors moves with the frames)
        self.recipe_standin = recipe.standin
        self.bar_base = np.minimum(np.array(self.standin), np.array(recipe.standin))

    def errors(self, got_f0, got_per, got_loud):
        """([3][N] errors of a result against float64, [3][N] bars): periodicity, cents, loudness in dB; the open frames against
        the nearest of their admissible answers."""
        err, want = frame_errors(got_f0, got_per, got_loud, self.t64, self.lag_open, self.den_open, self.guard)
        units = np.stack([np.abs(want[0]), np.full(self.t64.n, 1200.0 / np.log(2.0)), np.abs(want[2])]) * HALF_UNIT
        return err, BAR_FACTOR * np.maximum(self.bar_base[:, None], units)

    def not_admissible(self, got_f0, got_per):
        """The open frames whose answer is none of those their admissible lags give, within the bars."""
        _, bars = self.errors(self.t64.f0_raw, self.t64.per_raw, self.t64.loud)
        return [int(f) for f in np.nonzero(self.open)[0]
                if not admissible(got_f0, got_per, f, self.t64, self.guard, bars[0, f], bars[1, f])]


@functools.lru_cache(maxsize=None)
def sweep():
    return EdgeSet(SWEEP, cases())


@functools.lru_cache(maxsize=None)
def low_tones():
    return EdgeSet(LOW_POOL, cases(), sure_only=True)


TIE_LAGS = (31, 35, 36, 97, 319, 320)           # the first and the last lag of a lane (the neighbour comes from another lane), the range's end


def tie_clip(lag):
    """One frame of zeros with one sample of 0.5 at 703 + lag.  Every number of the search is exact in any precision: d is 0 up to
    the lag and 0.25 behind it, so d' is 1 (the rule for a running sum of 0) up to the lag, lag + 1 at lag + 1, and falls from
    there towards 1 without a local minimum.  Under a threshold over 1 the one candidate is the lag itself, on d'(lag) <=
    d'(lag - 1) with both sides equal and d'(lag) < d'(lag + 1); the parabola gives off = -0.5 and a periodicity clipped to 1.
    (At lag 320 the right neighbour is d'(321).)  A search that wants d'(lag) < d'(lag - 1) finds no candidate and falls back to
    lag 30, the smallest lag at the minimum."""
    x = np.zeros(WIN, np.float32)
    x[TERMS + lag] = 0.5
    return x


def pr_zero_pair():
    """(reference, estimate), 34 frames: a sweep-like tone of 2400 samples and 4000 of near-silence, in the two orders.  The reference
    is voiced in its first frames only and the estimate in its last: TP = 0, FP > 0, FN > 0."""
    tone_, quiet = edge_tone(100.3, 7, 3, T=2400), (1e-5 * np.random.default_rng(9).standard_normal(4000)).astype(np.float32)
    return np.concatenate([tone_, quiet]), np.concatenate([quiet, tone_])
