"""The K-weighting, the R 128 meter and the gain kernels over the whole range of rates (csrc/loudness.hip, csrc/r128.hip), through
the C ABI, against the float64 definitions of tests/loudness_ref.py and tests/r128_ref.py and under an fp64-scale bound.

Why.  The chunked evaluation of the recurrence is hardest at high rates: the high pass's poles sit at about 1 - 6e-4 at 192 kHz
and M^64 = A^8192, which carries the state across a group of 64 chunks, has entries of order 0.3 there (10^-33 at 24 kHz).  The
bound the other files use (loudness_ref.bound: the error of a sequential fp32 lfilter) is loosest exactly there: 10^-2 LU for
content under the high pass at 96 kHz and above.

Bound (loudness_ref.bound64): two fp32 ulps of the float64 value plus four times what a float64 stand-in of the chunked
evaluation (loudness_ref.weighted_chunked: plain numpy, its own order inside a step) differs from the sequential float64 lfilter
by, for the same quantity of the same clip.  The stand-in's error is measured per clip, printed and nowhere written down; that
four times it stays under ONE fp32 ulp of every value is asserted, so the bar is never wider than three ulps.  No block lies
within 0.01 LU of a loudness gate and no window within 10^-3 LU of a range gate in the reference (asserted): no gate can flip.

wt_loudness: at 8000, 48000, 88200, 96000, 176400, 192000 Hz and, with an uneven 100 ms grid, 8001, 11025, 44101, 47999, 191999
Hz: noise of 1.5 s, 30 Hz + DC of 1.5 s, a stereo clip whose channels lie more than n apart, noise of floor(4 fs / 10) - 1, + 0,
+ 1 samples (no block, one, one); at 192 kHz 30 Hz + DC of 3.5 s (5250 chunks: more than 64 groups, the scan loads a second batch
of totals with a carry that matters); at 24 kHz the low clip of tests/test_loudness_op.py.  One call per rate, and every clip alone.
wt_loudness_range: at 44100, 48000, 96000, 191999, 192000 Hz stepped noise of floor(30 fs / 10) - 1 and + 0 samples (no window,
one) and 4 s rising by 3 dB every 0.4 s (11 windows, all different), one of them stereo.
wt_true_peak: at 48000, 88200, 95999 (F = 4), 96000, 191999 (F = 2) and 192000 Hz (F = 1) the lengths 7, T + 1, 2 T + 3 and fs / 4
sines at 45 and 67.5 degrees, which neighbouring factors read differently by 10^4 times the bound.
wt_normalize_rows_lufs(_tp) at 48000, 96000, 192000 Hz, three rows; one call of 257 rows at 8000 Hz; the Python layer at 96000 Hz.
Measured on an MI355X: profiles/r128_rates_error.txt."""
import math

import numpy as np
import pytest
import torch

from tests import loudness_ref as R
from tests import r128_ref as Q

pytestmark = pytest.mark.gpu

SENTINEL = R.SENTINEL
EVEN = (8000, 48000, 88200, 96000, 176400, 192000)
UNEVEN = (8001, 11025, 44101, 47999, 191999)
RANGE_RATES = (44100, 48000, 96000, 191999, 192000)
PEAK_RATES = (48000, 88200, 95999, 96000, 191999, 192000)
GAIN_RATES = (48000, 96000, 192000)
AMPLITUDES = (0.3, 0.02, 1.7)
LEVELS = (-20.0, -26.0, -23.0, -31.0, -21.0, -28.0)
RISING = (-40.0, -37.0, -34.0, -31.0, -28.0, -25.0, -22.0, -19.0, -16.0, -13.0)
TARGET, CEILING = -23.0, -1.0


def _chunk():
    from wavtokenizer_amd import _capi
    return int(_capi.lib.wt_loudness_chunk())


def _tile():
    from wavtokenizer_amd import _capi
    return int(_capi.lib.wt_true_peak_tile())


def _upload(x: np.ndarray) -> torch.Tensor:
    """x on the GPU; two channels as a view into planes five floats longer than the clip (NaN between them)."""
    if x.ndim == 1:
        return torch.from_numpy(x).cuda()
    buf = torch.full((x.shape[0], x.shape[1] + 5), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return buf[:, :x.shape[1]]


def _err(got, want: float) -> float:
    return abs(float(got) - want) if math.isfinite(want) else 0.0


def _margin(ref) -> float:
    """The least distance of a block from either gate, in LU (loudness_ref.gate_margin on a result at hand)."""
    _L, gamma, _count, l = ref
    l = l[np.isfinite(l)]
    if l.size == 0:
        return math.inf
    d = float(np.abs(l + 70.0).min())
    return min(d, float(np.abs(l - gamma).min())) if math.isfinite(gamma) else d


class Clip:
    """A clip with the definition in float64 (ref), the same through the stand-in of the chunked evaluation (alt) and through a
    sequential fp32 lfilter (f32: printed beside the bar, it bounds nothing here)."""

    def __init__(self, name, fs, x):
        self.name, self.fs, self.x, self.n = name, fs, x, x.shape[-1]
        self.ref = R.loudness(x, fs)
        self.alt = R.loudness(x, fs, y=R.weighted_chunked(x, fs, _chunk()))
        self.f32 = R.loudness(x, fs, np.float32)

    def values(self):
        """(want, stand-in) of L, the threshold and every momentary value."""
        return [(self.ref[0], self.alt[0]), (self.ref[1], self.alt[1])] + list(zip(self.ref[3], self.alt[3]))


def _loudness_clips():
    out = []
    for r, fs in enumerate(EVEN + UNEVEN):
        seed = 7300 + 20 * r
        n = fs * 3 // 2
        out.append(Clip("noise", fs, R.make_clip(n, seed=seed, amplitude=AMPLITUDES[r % 3])))
        out.append(Clip("low", fs, R.make_low_clip(n, fs, seed=seed + 1)))
        out.append(Clip("stereo", fs, np.stack([R.make_clip(fs + 13, seed=seed + 2, amplitude=0.3), R.make_clip(fs + 13, seed=seed + 3, amplitude=0.1)])))
        for k in (-1, 0, 1):
            out.append(Clip("edge%+d" % k, fs, R.make_clip(4 * fs // 10 + k, seed=seed + 5 + k, amplitude=AMPLITUDES[(r + k) % 3])))
    out.append(Clip("low3.5s", 192000, R.make_low_clip(672000, 192000, seed=7290)))
    out.append(Clip("low", 24000, R.make_low_clip(72000, 24000, seed=7118)))               # the `low` clip of tests/test_loudness_op.py
    out.append(Clip("noise", 24000, R.make_clip(36000, seed=7291)))
    return out


@pytest.fixture(scope="module")
def clips():
    """Every wt_loudness clip on the CPU with its references, computed once and left unchanged."""
    return _loudness_clips()


@pytest.fixture(scope="module")
def measured(clips):
    """Per clip (out (3,), l_j) from the one call of its rate, and the same from a call of its own."""
    got = [None] * len(clips)
    for fs in sorted({c.fs for c in clips}):
        idx = [j for j, c in enumerate(clips) if c.fs == fs]
        on_gpu = [_upload(clips[j].x) for j in idx]
        assert all(t.dim() == 1 or t.stride(0) > t.shape[1] for t in on_gpu)
        out, blocks = R.measure(on_gpu, fs)
        for r, j in enumerate(idx):
            o1, b1 = R.measure([on_gpu[r]], fs)
            got[j] = (out[r], blocks[r], o1[0], b1[0])
    return got


def test_the_references_conditions_hold(clips):
    """What the GPU tests below rest on, for the references alone."""
    C = _chunk()
    worst = 0.0
    for c in clips:
        assert _margin(c.ref) >= 0.01, (c.name, c.fs, _margin(c.ref))
        assert c.ref[2] == c.alt[2] == c.f32[2] and len(c.ref[3]) == len(c.alt[3]), (c.name, c.fs)
        if c.name.startswith("edge"):
            assert len(c.ref[3]) == c.ref[2] == (0 if c.name == "edge-1" else 1), (c.name, c.fs)
        else:
            assert c.ref[2] > 0, (c.name, c.fs)
        for want, alt in c.values():                            # the bar is under three ulps: four times the stand-in's error is under one
            if math.isfinite(want):
                assert 4.0 * abs(alt - want) < R.ulp32(want), (c.name, c.fs, want, alt)
                worst = max(worst, 4.0 * abs(alt - want) / R.ulp32(want))
    long = next(c for c in clips if c.name == "low3.5s")
    assert -(-long.n // C) > 64 * 64, C                         # more than 64 groups of 64 chunks (5250 chunks of 128)
    print(f"rates_error worst 4 x stand-in error / ulp {worst:.3f}")


def test_loudness_threshold_count_and_momentary_within_bound64(clips, measured):
    from wavtokenizer_amd import _capi
    worst, worst_abs = 0.0, 0.0
    for c, (out, blocks, _o1, _b1) in zip(clips, measured):
        L, G, count, l = c.ref
        bar_L, bar_G = R.bound64(L, c.alt[0]), R.bound64(G, c.alt[1])
        err_l = [_err(g, w) for g, w in zip(blocks, l)]
        bar_l = [R.bound64(w, a) for w, a in zip(l, c.alt[3])]
        ratio_l = max((e / b for e, b in zip(err_l, bar_l) if b > 0), default=0.0)
        print(f"rates_error {c.name:8s} fs {c.fs:6d} n {c.n:7d} ch {c.x.ndim}  L {float(out[0]):12.6f}  err {_err(out[0], L):.3e}  bar {bar_L:.3e}  "
              f"stand-in err {_err(c.alt[0], L):.3e}  fp32 lfilter err {_err(c.f32[0], L):.3e}  threshold err {_err(out[1], G):.3e}  "
              f"blocks {int(out[2])}/{len(l)}  momentary worst err {max(err_l, default=0.0):.3e}  worst err / bar {ratio_l:.3f}")
        assert blocks.shape == l.shape and len(l) == int(_capi.lib.wt_loudness_blocks(c.n, c.fs)), (c.name, c.fs)
        if not math.isfinite(L):
            assert out[0] == -np.inf and out[1] == -np.inf and out[2] == 0, (c.name, c.fs)
        else:
            assert _err(out[0], L) <= bar_L, (c.name, c.fs, float(out[0]), L, bar_L)
            assert _err(out[1], G) <= bar_G, (c.name, c.fs, float(out[1]), G, bar_G)
            assert float(out[2]) == count, (c.name, c.fs, out[2], count)
            worst = max(worst, _err(out[0], L) / bar_L, _err(out[1], G) / bar_G)
            worst_abs = max(worst_abs, _err(out[0], L))
        for j, (g, w, e, b) in enumerate(zip(blocks, l, err_l, bar_l)):
            assert (g == w) if not math.isfinite(w) else (e <= b), (c.name, c.fs, j, float(g), w, b)
        worst = max(worst, ratio_l)
    print(f"rates_error worst |L - L64| {worst_abs:.3e} LU, worst err / bar {worst:.3f}")


def test_a_clip_has_the_same_bits_alone_and_in_its_rates_batch(clips, measured):
    for c, (out, blocks, o1, b1) in zip(clips, measured):
        assert out.tobytes() == o1.tobytes() and blocks.tobytes() == b1.tobytes(), (c.name, c.fs)


# ---- loudness range ----------------------------------------------------------------------------------------------------------------
class RangeClip:
    def __init__(self, name, fs, x):
        self.name, self.fs, self.x, self.n = name, fs, x, x.shape[-1]
        self.z, self.s = Q.short_term(x, fs, y=R.weighted(x, fs))
        self.z_alt, self.s_alt = Q.short_term(x, fs, y=R.weighted_chunked(x, fs, _chunk()))
        self.lra, self.lo, self.hi, self.m, self.rel, self.margin = Q.loudness_range(self.z)
        _lra, self.lo_alt, self.hi_alt, self.m_alt, _rel, _margin_alt = Q.loudness_range(self.z_alt)


def _range_clips():
    out = []
    for r, fs in enumerate(RANGE_RATES):
        seed = 9600 + 10 * r
        for k in (-1, 0):
            out.append(RangeClip("edge%+d" % k, fs, Q.make_stepped(30 * fs // 10 + k, fs, seed + 1 + k, LEVELS, 0.5)))
        x = Q.make_stepped(4 * fs, fs, seed + 2, RISING, 0.4)
        if fs == 96000:
            x = np.stack([x, Q.make_stepped(4 * fs, fs, seed + 3, RISING, 0.4)])
        out.append(RangeClip("rising", fs, x))
    return out


@pytest.fixture(scope="module")
def range_clips():
    """Every wt_loudness_range clip on the CPU with its references, computed once and left unchanged."""
    return _range_clips()


@pytest.fixture(scope="module")
def range_measured(range_clips):
    """Per clip {"batch", "alone"}: ((9,), l_j, s_j) each, and "loudness": wt_loudness's ((3,), l_j)."""
    got = [dict() for _ in range_clips]
    for fs in RANGE_RATES:
        idx = [j for j, c in enumerate(range_clips) if c.fs == fs]
        on_gpu = [_upload(range_clips[j].x) for j in idx]
        out, mom, sht = Q.measure_range(on_gpu, fs)
        lout, lblocks = R.measure(on_gpu, fs)
        for r, j in enumerate(idx):
            got[j]["batch"] = (out[r], mom[r], sht[r])
            got[j]["loudness"] = (lout[r], lblocks[r])
            o1, m1, s1 = Q.measure_range([on_gpu[r]], fs)
            got[j]["alone"] = (o1[0], m1[0], s1[0])
    return got


def test_the_range_references_conditions_hold(range_clips):
    for c in range_clips:
        assert c.margin >= 1e-3, (c.name, c.fs, c.margin)
        assert c.m == c.m_alt, (c.name, c.fs)
        assert len(c.s) == c.m == {"edge-1": 0, "edge+0": 1, "rising": 11}[c.name], (c.name, c.fs, len(c.s), c.m)
        pairs = list(zip(c.s, c.s_alt)) + ([(c.lo, c.lo_alt), (c.hi, c.hi_alt)] if c.m else [])
        for want, alt in pairs:
            assert 4.0 * abs(alt - want) < R.ulp32(want), (c.name, c.fs, want, alt)
        if c.name == "rising":                                  # the windows differ by far more than their bars
            assert float(np.diff(np.sort(c.s)).min()) > 1e-2 and c.lra > 3.0, (c.fs, c.s)


def test_short_term_low_high_range_and_count_within_bound64(range_clips, range_measured):
    from wavtokenizer_amd import _capi
    worst = 0.0
    for c, g in zip(range_clips, range_measured):
        out, _mom, sht = g["batch"]
        assert len(sht) == len(c.s) == int(_capi.lib.wt_short_term_blocks(c.n, c.fs)), (c.name, c.fs)
        err_s = [_err(a, w) for a, w in zip(sht, c.s)]
        bar_s = [R.bound64(w, a) for w, a in zip(c.s, c.s_alt)]
        for j, (e, b) in enumerate(zip(err_s, bar_s)):
            assert e <= b, (c.name, c.fs, j, e, b)
            worst = max(worst, e / b)
        assert int(out[6]) == c.m, (c.name, c.fs, out[6], c.m)
        if c.m == 0:
            assert np.isnan(out[3]) and np.isnan(out[4]) and np.isnan(out[5]) and out[8] == -np.inf, (c.name, c.fs)
            print(f"rates_error range {c.name:7s} fs {c.fs:6d} n {c.n:7d} ch {c.x.ndim}  S {len(sht):3d}  no range")
            continue
        b_lo, b_hi = R.bound64(c.lo, c.lo_alt), R.bound64(c.hi, c.hi_alt)
        b_lra = b_lo + b_hi + R.ulp32(c.lra)
        print(f"rates_error range {c.name:7s} fs {c.fs:6d} n {c.n:7d} ch {c.x.ndim}  S {len(sht):3d}  short-term worst err {max(err_s):.3e}  bar {min(bar_s):.3e}  "
              f"stand-in err {max(_err(a, w) for w, a in zip(c.s, c.s_alt)):.3e}  LRA {float(out[3]):9.5f} LU  err {_err(out[3], c.lra):.3e}  "
              f"bar {b_lra:.3e}  low {float(out[4]):9.4f} err {_err(out[4], c.lo):.3e}  high {float(out[5]):9.4f} err {_err(out[5], c.hi):.3e}  "
              f"m {int(out[6])}  margin {c.margin:.2e}")
        assert _err(out[4], c.lo) <= b_lo, (c.name, c.fs, out[4], c.lo)
        assert _err(out[5], c.hi) <= b_hi, (c.name, c.fs, out[5], c.hi)
        assert _err(out[3], c.lra) <= b_lra, (c.name, c.fs, out[3], c.lra)
        assert out[8].tobytes() == sht.max().tobytes(), (c.name, c.fs)
        worst = max(worst, _err(out[4], c.lo) / b_lo, _err(out[5], c.hi) / b_hi, _err(out[3], c.lra) / b_lra)
    print(f"rates_error range worst err / bar {worst:.3f}")


def test_range_call_has_the_bits_of_wt_loudness_and_the_same_alone(range_clips, range_measured):
    for c, g in zip(range_clips, range_measured):
        out, mom, _sht = g["batch"]
        lout, lblocks = g["loudness"]
        assert out[:3].tobytes() == lout.tobytes() and mom.tobytes() == lblocks.tobytes(), (c.name, c.fs)
        assert np.isfinite(out[0]) and out[7].tobytes() == mom.max().tobytes(), (c.name, c.fs)
        for a, b in zip(g["alone"], g["batch"]):
            assert a.tobytes() == b.tobytes(), (c.name, c.fs)


# ---- true peak ---------------------------------------------------------------------------------------------------------------------
def _sine(n: int, phase: float) -> np.ndarray:
    """fs / 4 of amplitude 0.5 (n a multiple of 4: whole periods).  At 45 degrees every sample is +-0.354 and the peaks lie half
    way between two: F = 2 and F = 4 find them, F = 1 does not.  At 67.5 degrees the peaks lie a quarter of the way: F = 4 finds
    them, F = 2 lands on +-0.462 again, where the samples are."""
    return (0.5 * np.sin(2 * np.pi * 0.25 * np.arange(n) + math.radians(phase))).astype(np.float32)


def test_true_peak_on_either_side_of_the_factor_switches():
    T = _tile()
    worst = 0.0
    for r, fs in enumerate(PEAK_RATES):
        F = Q.factor(fs)
        assert F == {48000: 4, 88200: 4, 95999: 4, 96000: 2, 191999: 2, 192000: 1}[fs]
        xs = [R.make_clip(n, seed=8300 + 10 * r + k, amplitude=AMPLITUDES[(r + k) % 3]) for k, n in enumerate((7, T + 1, 2 * T + 3))]
        xs += [_sine(2 * T + 4, 45.0), _sine(2 * T + 4, 67.5)]
        got = Q.measure_true_peak([torch.from_numpy(x).cuda() for x in xs], fs)
        for x, g in zip(xs, got):
            tp, sp, bound = Q.true_peak(x, fs)
            err = abs(float(g[0]) - tp)
            print(f"rates_error true_peak fs {fs:6d} F {F} n {x.shape[0]:5d}  dBTP {Q.db(float(g[0])):9.4f}  sample {Q.db(float(g[1])):9.4f} dBFS  "
                  f"err {err:.3e}  bound {bound:.3e}")
            assert err <= bound, (fs, x.shape[0], err, bound)
            assert float(g[1]) == sp and g[0] >= g[1], (fs, x.shape[0])
            worst = max(worst, err / bound if bound > 0 else 0.0)
        # the sines tell the factors apart: the neighbouring factor reads them differently by far more than the bound
        for x, g, others in ((xs[-1], got[-1], {4: 2, 2: 4}), (xs[-2], got[-2], {2: 1, 1: 2})):
            if F not in others:
                continue
            tp, sp, bound = Q.true_peak(x, fs)
            tp_other, _sp, bound_other = Q.true_peak(x, fs, F=others[F])
            assert abs(tp - tp_other) > 0.02 > 1000.0 * max(bound, bound_other), (fs, tp, tp_other)
            assert abs(float(g[0]) - tp_other) > 0.02, (fs, float(g[0]), tp_other)
        if F == 1:
            assert all(g[0].tobytes() == g[1].tobytes() for g in got)
        else:
            tp, sp, _bound = Q.true_peak(xs[-2], fs)
            assert tp - sp > 0.1 and float(got[-2][0]) - float(got[-2][1]) > 0.1, (fs, got[-2])      # 0.5 against 0.354
    print(f"rates_error true_peak worst err / bound {worst:.3f}")


# ---- the gain kernels ------------------------------------------------------------------------------------------------------------------
def _clicked(n: int, seed: int, where: int) -> np.ndarray:
    """Quiet noise with a click two samples wide: its true peak lies between them where the rate is oversampled."""
    x = R.make_clip(n, seed=seed, amplitude=0.003)
    x[where:where + 2] = 0.5
    return x


def _d_L_tolerance(c: Clip) -> float:
    return (math.log(10.0) / 20.0) * R.bound64(c.ref[0], c.alt[0]) + 2.0 ** -23


@pytest.mark.parametrize("fs", GAIN_RATES)
def test_gain_kernels(fs):
    seed = 9700 + fs // 1000
    quiet = Clip("quiet", fs, _clicked(6 * fs // 10 + 1, seed, fs // 5))
    plain = Clip("plain", fs, R.make_clip(fs // 2 + 3, seed=seed + 1, amplitude=0.1))
    short = R.make_clip(4 * fs // 10 - 1, seed=seed + 2, amplitude=0.3)
    short[100] = 2.0
    xs, lens = [quiet.x, plain.x, short], [quiet.n, plain.n, short.shape[0]]
    T_pad = max(lens) // 4 * 4 + 7
    assert T_pad % 4 == 3 and R.blocks(lens[2], fs) == 0
    ceiling = 10.0 ** (CEILING / 20.0)
    want_L = [10.0 ** ((c.ref[0] - TARGET) / 20.0) for c in (quiet, plain)]
    peaks = [Q.true_peak(c.x, fs) for c in (quiet, plain)]
    want_P = [p[0] / ceiling for p in peaks]
    for c in (quiet, plain):                                    # the references' conditions
        assert _margin(c.ref) >= 0.01 and c.ref[2] == c.alt[2] > 0, (fs, c.name)
        assert 4.0 * abs(c.alt[0] - c.ref[0]) < R.ulp32(c.ref[0]), (fs, c.name)
    assert want_P[0] > 2.0 * want_L[0] and want_L[1] > 1.2 * want_P[1] and abs(want_L[1] - 1.0) > 0.01, (fs, want_L, want_P)
    if Q.factor(fs) > 1:
        assert peaks[0][0] > 1.1 * peaks[0][1]                  # the click's true peak is not its sample peak
    else:
        assert peaks[0][0] == peaks[0][1] == 0.5

    def run(call):
        rows = torch.full((3, T_pad), SENTINEL, dtype=torch.float32, device="cuda")
        for r, x in enumerate(xs):
            rows[r, :lens[r]] = torch.from_numpy(x).cuda()
        scales = call(rows).cpu().numpy()
        rows = rows.cpu().numpy()
        assert scales.dtype == np.float32
        for r, x in enumerate(xs):
            assert rows[r, :lens[r]].tobytes() == (x / scales[r]).astype(np.float32).tobytes(), (fs, r)      # one IEEE division per sample
            assert bool((rows[r, lens[r]:] == SENTINEL).all()), (fs, r)
        assert scales[2] == 1.0 and rows[2, :lens[2]].tobytes() == short.tobytes(), fs                       # no loudness: untouched
        return scales

    free = run(lambda rows: R.normalize_rows_lufs(rows, lens, fs, TARGET))
    held = run(lambda rows: Q.normalize_rows_lufs_tp(rows, lens, fs, TARGET, CEILING))
    for r, c in enumerate((quiet, plain)):
        print(f"rates_error gain fs {fs:6d} {c.name}  d_L {float(free[r]):.7f}  want {want_L[r]:.7f}  rel err {abs(float(free[r]) - want_L[r]) / want_L[r]:.3e}  "
              f"tol {_d_L_tolerance(c):.3e}  under the ceiling {float(held[r]):.7f}  TP / ceiling {want_P[r]:.7f}")
        assert abs(float(free[r]) - want_L[r]) <= _d_L_tolerance(c) * want_L[r], (fs, c.name, float(free[r]), want_L[r])
        assert free[r] != 1.0
    # scale = max(d_L, fp32(true peak / ceiling)): the quiet row's is the true peak's (within its bound and the two roundings), the plain row's d_L
    assert abs(float(held[0]) - want_P[0]) <= peaks[0][2] / ceiling + 2.0 ** -23 * want_P[0], (fs, float(held[0]), want_P[0])
    assert held[1].tobytes() == free[1].tobytes(), fs


def test_257_rows_have_the_bits_of_their_batches_of_three():
    """More rows than loud_ceiling_kernel has threads in a workgroup: rows 0, 255 and 256 are the ones the ceiling binds."""
    fs, n, B = 8000, 4000, 257
    clicked = (0, 255, 256)
    xs = [_clicked(n, 9800 + r, 500 + 7 * r) if r in clicked else R.make_clip(n, seed=9800 + r, amplitude=0.05 + 0.001 * (r % 50)) for r in range(B)]
    ceiling = 10.0 ** (CEILING / 20.0)
    assert R.blocks(n, fs) == 2
    all_rows = torch.full((B, n + 3), SENTINEL, dtype=torch.float32, device="cuda")
    all_rows[:, :n] = torch.from_numpy(np.stack(xs)).cuda()
    start = all_rows.clone()
    scales = Q.normalize_rows_lufs_tp(all_rows, [n] * B, fs, TARGET, CEILING)
    assert bool((all_rows[:, n:] == SENTINEL).all())
    for r in clicked:
        tp, _sp, bound = Q.true_peak(xs[r], fs)
        d_L = 10.0 ** ((R.loudness(xs[r], fs)[0] - TARGET) / 20.0)
        assert tp / ceiling > 2.0 * d_L
        assert abs(float(scales[r]) - tp / ceiling) <= bound / ceiling + 2.0 ** -23 * tp / ceiling, (r, float(scales[r]), tp / ceiling)
    assert bool((scales != 1.0).all())
    seen = torch.zeros(B, dtype=torch.bool)
    for r0 in list(range(0, B - 3, 3)) + [B - 3]:
        rows = start[r0:r0 + 3].clone()
        s3 = Q.normalize_rows_lufs_tp(rows, [n] * 3, fs, TARGET, CEILING)
        assert torch.equal(rows, all_rows[r0:r0 + 3]), r0
        assert s3.cpu().numpy().tobytes() == scales[r0:r0 + 3].cpu().numpy().tobytes(), r0
        seen[r0:r0 + 3] = True
    assert bool(seen.all())


def test_the_python_layer_at_96_khz(clips, measured, range_clips, range_measured):
    from wavtokenizer_amd import audio
    fs = 96000

    def bits(t):
        return t.detach().cpu().numpy().tobytes()

    for name in ("noise", "low", "stereo"):
        j = next(j for j, c in enumerate(clips) if c.fs == fs and c.name == name)
        assert bits(audio.loudness(_upload(clips[j].x), sample_rate=fs)) == measured[j][0].tobytes(), name
    j = next(j for j, c in enumerate(range_clips) if c.fs == fs and c.name == "rising")
    out, mom, sht = audio.loudness_range(_upload(range_clips[j].x), sample_rate=fs, series=True)
    want = range_measured[j]["batch"]
    assert range_clips[j].x.ndim == 2 and bits(out) == want[0].tobytes() and bits(mom) == want[1].tobytes() and bits(sht) == want[2].tobytes()
    x = torch.from_numpy(_sine(2 * _tile() + 4, 45.0)).cuda()
    lin = Q.measure_true_peak([x], fs)
    got = audio.true_peak(x, sample_rate=fs)
    assert bits(got) == bits(20.0 * torch.log10(torch.from_numpy(lin[0]).cuda()))
    tp, sp, bound = Q.true_peak(x.cpu().numpy(), fs)
    assert abs(float(lin[0, 0]) - tp) <= bound and float(lin[0, 1]) == sp and tp > 1.3 * sp      # F = 2 finds the peak between the samples
