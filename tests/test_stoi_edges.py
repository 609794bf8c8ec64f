"""The STOI kernels (csrc/stoi.hip) at their degenerate and structural edges, at 10 kHz where no resampler blurs the sample
positions (the gain test alone also runs at 24 kHz):
    exact zeros          a zero processed signal, a zero clean signal and both: 0.0 exactly, no NaN; the + EPS terms (2^-52, far below
                         fp32's ulp of 1) are all that stands between the kernels and 0 / 0
    a gated clean signal exact zeros inside a clip: frames of zero energy among the candidates
    the select kernel    K0 = 255, 256, 257 around its chunk of 256 frames, with gaps in the kept-frame list
    the packing          8 and 9 segments (the segment kernel's 8 per block), 64 and 65 (the mean kernel's stride)
    influence            a sample that lies in dropped frames alone moves no bit; one in a kept frame moves exactly the columns of the
                         silence-removed frames that hold it
    gain                 a power-of-two gain on both signals, or on the processed one alone, moves no bit
The conditioned cases are compared with the float64 definition (tests/stoi_ref.py) by the statistics and rules of
tests/test_stoi_op.py; the bars are 4 x the worst deviation the fp32 stand-in reaches over this module's conditioned cases, computed
on the CPU here, never from the kernel.  Measured on an MI355X: profiles/stoi_error.txt."""
import functools

import numpy as np
import pytest

from tests import stoi_ref as R
from tests.test_stoi_op import _deviations, _shaped

pytestmark = pytest.mark.gpu

FS = R.FS
GAINS = (2.0 ** -12, 2.0 ** 9)


def _quiet(T, seed, stretches):
    """speechlike with the sample ranges of `stretches` at gain 1e-4."""
    g = np.ones(T)
    for lo, hi in stretches:
        g[lo:hi] = 1e-4
    return (R.speechlike(T, FS, seed).astype(np.float64) * g).astype(np.float32)


def _base():
    x = R.speechlike(6000, FS, 30)
    return x, R.noisy(x, 0)


def _gated():
    x, y = _base()
    x = x.copy()
    x[2000:3500] = 0.0
    return x, y


# the select kernel's chunk: one silent stretch over frames 61..199 (frames 60 and 200 partly), which leaves waves 1 and 2 of the
# chunk without a kept frame, and two stretches (frames 41..89 and 151..209) that leave kept frames in all four waves
ONE_STRETCH = ((7808, 25728),)
TWO_STRETCHES = ((5248, 11648), (19328, 26880))
CHUNK = {255: 32896, 256: 33024, 257: 33152}
PACKING = {38: 4993, 39: 5121, 94: 12161, 95: 12289}               # contiguous clips: K = K0, K - 30 segments


def _cases():
    """name: (rate, clean, processed, SNR in dB); every pair here is conditioned (asserted in reference())."""
    out = {"6000 samples": (FS,) + _base() + (0,), "gated clean signal": (FS,) + _gated() + (0,)}
    for i, (k0, T) in enumerate(CHUNK.items()):
        for j, (tag, st) in enumerate((("one silent stretch", ONE_STRETCH), ("two silent stretches", TWO_STRETCHES))):
            x = _quiet(T, 40 + 2 * i + j, st)
            out[f"K0 = {k0}, {tag}"] = (FS, x, R.noisy(x, (20, 0, -10)[i], seed=40 + i), (20, 0, -10)[i])
    for i, (k, T) in enumerate(PACKING.items()):
        x = R.speechlike(T, FS, 50 + i)
        out[f"K = {k}: {k - 30} segments"] = (FS, x, R.noisy(x, (20, 0, -10)[i % 3], seed=50 + i), (20, 0, -10)[i % 3])
    x = _shaped(20000, FS, 60, "middle")
    out["silent middle third"] = (FS, x, R.noisy(x, 0, seed=60), 0)
    for fs in (FS, 24000):
        x = R.speechlike(3 * fs, fs, 70)
        out[f"3 s at {fs} Hz"] = (fs, x, R.noisy(x, 0, seed=70), 0)
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """Per conditioned case: (rate, x, y, float64 stages, SNR), the conditions asserted; the four bars.  CPU only."""
    out = {}
    worst = dict(res=0.0, band=0.0, d=0.0, e=0.0)
    for name, (fs, x, y, snr) in _cases().items():
        s64 = R.stages(x.astype(np.float64), y.astype(np.float64), fs)
        assert s64.K0 == R.candidate_frames(R.resampled_length(len(x), fs))
        margin = R.keep_margin(s64)
        assert margin >= 1e-3, (name, margin)
        assert min(s64.cond.values()) >= 1e-3, (name, s64.cond)
        s32 = R.stages(x, y, fs, np.float32, keep=s64.keep)
        dev = _deviations(s32, s64, fs)
        for k in worst:
            worst[k] = max(worst[k], dev[k])
        out[name] = (fs, x, y, s64, snr)
    # what the cases are there for
    s = out["6000 samples"][3]
    assert (s.K0, s.K) == (45, 45)
    s = out["gated clean signal"][3]
    assert (s.K0, s.K) == (45, 35) and bool((s.norms == 0.0).any())
    for k0 in CHUNK:
        for tag in ("one silent stretch", "two silent stretches"):
            s = out[f"K0 = {k0}, {tag}"][3]
            assert s.K0 == k0 and 31 < s.K < k0 - 80, (k0, tag, s.K)
            assert s.keep[:30].all() and s.keep[220:].all() and not s.keep[61:90].any() and not s.keep[151:200].any()
        assert all(out[f"K0 = {k0}, two silent stretches"][3].keep[64 * w: 64 * w + 64].any() for w in range(4))
    assert out["K0 = 257, one silent stretch"][3].keep[256] and out["K0 = 257, two silent stretches"][3].keep[256]
    for k in PACKING:
        s = out[f"K = {k}: {k - 30} segments"][3]
        assert (s.K0, s.K) == (k, k)
    s = out["silent middle third"][3]
    assert s.K > 60 and np.diff(np.nonzero(s.keep)[0]).max() > 20
    bars = {k: 4.0 * v for k, v in worst.items()}
    print("stoi_error stand-in (fp32, sequential sums, radix-2 FFT, CPU) over tests/test_stoi_edges.py: worst resampled %.3e  bands %.3e  "
          "STOI %.3e  ESTOI %.3e; the bars are 4 x these" % (worst["res"], worst["band"], worst["d"], worst["e"]))
    # (the yardstick itself: fp32 rounding, not a broken stand-in)
    assert 1e-8 < worst["res"] < 1e-5 and 1e-8 < worst["band"] < 1e-4 and 0 < worst["d"] < 1e-4 and 0 < worst["e"] < 1e-4
    return out, bars


@pytest.fixture(scope="module")
def ref():
    return reference()


def _both(xs, ys, fs):
    """One STOI and one ESTOI call with taps on the pairs: (the STOI call's clips, d [n], e [n]); the stages must not depend on the
    measure, nothing outside the outputs may be written."""
    plain = R.run(xs, ys, fs, extended=False)
    ext = R.run(xs, ys, fs, extended=True)
    assert plain.intact and ext.intact
    for a, b in zip(plain.clips, ext.clips):
        for f in ("xr", "yr", "keep", "X", "Y"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert (a.K0, a.K) == (b.K0, b.K)
    return plain.clips, plain.d, ext.d


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _against_float64(ref, names, got):
    """The stage checks of tests/test_stoi_op.py on the cases `names`, got = (clips, d, e) of their launch."""
    cases, bars = ref
    clips, d, e = got
    bad = []
    for i, name in enumerate(names):
        fs, x, _y, s64, snr = cases[name]
        s = clips[i]
        assert (s.K0, s.K) == (s64.K0, s64.K), name
        assert np.array_equal(s.keep, s64.keep), name
        assert np.isfinite(d[i]) and np.isfinite(e[i]) and not np.isnan(s.X).any() and not np.isnan(s.Y).any(), name
        s.d = {False: d[i], True: e[i]}
        dev = _deviations(s, s64, fs)
        print(f"stoi_error {name:38s} {fs:5d} Hz T {len(x):6d} SNR {snr:3d}  K0 {s.K0:4d} K {s.K:4d}  STOI {float(d[i]):.6f} (float64 {s64.d[False]:.6f})  "
              f"ESTOI {float(e[i]):.6f} (float64 {s64.d[True]:.6f})  resampled {dev['res']:.2e} (bar {bars['res']:.2e})  "
              f"bands {dev['band']:.2e} (bar {bars['band']:.2e})  |d| {dev['d']:.2e} (bar {bars['d']:.2e})  |e| {dev['e']:.2e} (bar {bars['e']:.2e})")
        for k in ("res", "band", "d", "e"):
            if not dev[k] <= bars[k]:
                bad.append((name, k, dev[k], bars[k]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ exact zeros
@functools.lru_cache(maxsize=None)
def zero_pairs():
    """[(what, clean, processed)] and, on the CPU, what the definition and the stand-in make of them: exact zeros, no NaN."""
    x, y = _base()
    z = np.zeros_like(x)
    pairs = [("zero processed", x, z), ("zero clean", z, y), ("both zero", z, z)]
    for what, a, b in pairs:
        for dt in (np.float64, np.float32):
            with np.errstate(invalid="ignore", divide="ignore"):       # (the condition numbers of a zero row are 0 / 0: not used here)
                s = R.stages(a.astype(dt), b.astype(dt), FS, dt)
            assert (s.K0, s.K) == (45, 45), (what, dt)                 # both zero: 0 + EPS > 0.01 (0 + EPS) keeps every frame
            assert s.d[False] == 0.0 and s.d[True] == 0.0, (what, dt, s.d)
            assert not np.isnan(s.X).any() and not np.isnan(s.Y).any()
    return pairs


def test_exact_zeros(ref):
    cases, bars = ref
    pairs = zero_pairs()
    x, y = _base()
    xs = [p[1] for p in pairs] + [x, x]
    ys = [p[2] for p in pairs] + [x, y]
    clips, d, e = _both(xs, ys, FS)
    for i, (what, _a, _b) in enumerate(pairs):
        s = clips[i]
        assert (s.K0, s.K) == (45, 45) and s.keep.all(), what
        assert not np.isnan(s.X).any() and not np.isnan(s.Y).any(), what
        print(f"stoi_error {what:38s} {FS:5d} Hz T {len(x):6d}  K0 {s.K0:4d} K {s.K:4d}  STOI {float(d[i])!r}  ESTOI {float(e[i])!r}")
        assert d[i] == 0.0 and e[i] == 0.0, (what, d[i], e[i])
    # a signal against itself
    print(f"stoi_error {'a signal against itself':38s} {FS:5d} Hz T {len(x):6d}  |d - 1| {abs(float(d[3]) - 1.0):.2e} (bar {bars['d']:.2e})  "
          f"|e - 1| {abs(float(e[3]) - 1.0):.2e} (bar {bars['e']:.2e})")
    assert abs(R.stoi64(x, x, FS) - 1.0) <= 1e-9 and abs(R.stoi64(x, x, FS, True) - 1.0) <= 1e-9
    assert abs(float(d[3]) - 1.0) <= bars["d"] and abs(float(e[3]) - 1.0) <= bars["e"]
    # the conditioned neighbour: against float64, and the bits of its own call
    _against_float64(ref, ["6000 samples"], (clips[4:], d[4:], e[4:]))
    alone = _both([x], [y], FS)
    assert _same_bits(alone[1], d[4:]) and _same_bits(alone[2], e[4:])
    for f in ("keep", "X", "Y"):
        assert _same_bits(getattr(alone[0][0], f), getattr(clips[4], f)), f


# ------------------------------------------------------------------------------------------------ structure
def test_gated_clean_signal(ref):
    cases, _bars = ref
    _fs, x, y, _s64, _snr = cases["gated clean signal"]
    _against_float64(ref, ["gated clean signal"], _both([x], [y], FS))


def test_select_kernel_chunk_boundary(ref):
    cases, _bars = ref
    names = [n for n in cases if n.startswith("K0 = ")]
    assert len(names) == 6
    _against_float64(ref, names, _both([cases[n][1] for n in names], [cases[n][2] for n in names], FS))


def test_segment_and_mean_packing(ref):
    cases, _bars = ref
    names = [f"K = {k}: {k - 30} segments" for k in PACKING]
    _against_float64(ref, names, _both([cases[n][1] for n in names], [cases[n][2] for n in names], FS))


@functools.lru_cache(maxsize=None)
def eps_scale():
    """The gated pair scaled so that the loudest frame's norm is 99.5 and 98.5 times EPS: a frame of zeros is kept when
    0 + EPS > 0.01 (max + EPS), that is below 99 EPS and not above.  The one place where the EPS on the threshold's side decides
    (without it the line would lie at 100 EPS).  [(clean, processed, float64 keep mask)]; the stand-in agrees.  CPU only."""
    x, y = _gated()
    top = float(R._select(x.astype(np.float64), np.float64)[0].max())
    out = []
    for target, kept in ((99.5, 35), (98.5, 45)):
        a, b = ((v.astype(np.float64) * (target * R.EPS / top)).astype(np.float32) for v in (x, y))
        norms, keep = R._select(a.astype(np.float64), np.float64)
        assert abs(norms.max() / R.EPS - target) < 0.01 and int(keep.sum()) == kept and bool((norms == 0.0).sum() == 10)
        thr = R.RANGE * (norms.max() + R.EPS)
        assert float((np.abs(norms + R.EPS - thr) / thr).min()) >= 1e-3
        assert np.array_equal(R._select(a, np.float32)[1], keep)
        out.append((a, b, keep))
    return out


def test_keep_threshold_where_eps_decides():
    cases = eps_scale()
    clips, d, e = _both([c[0] for c in cases], [c[1] for c in cases], FS)
    for i, (_a, _b, keep) in enumerate(cases):
        assert np.array_equal(clips[i].keep, keep) and clips[i].K == int(keep.sum()), (i, clips[i].K, int(keep.sum()))
        assert np.isfinite(d[i]) and np.isfinite(e[i]) and not np.isnan(clips[i].X).any() and not np.isnan(clips[i].Y).any()


# ------------------------------------------------------------------------------------------------ influence
def _columns(kept, J, m):
    """The frames j < J of the silence-removed signal that hold sample m of the 10 kHz signal: kept frame number k (candidate frame
    kept[k]) gives its first half to frames k - 1 and k, its second half to frames k and k + 1."""
    cols = set()
    for k, f in enumerate(kept):
        o = m - R.HOP * int(f)
        if 0 <= o < R.FRAME:
            cols |= {k, k - 1} if o < R.HOP else {k, k + 1}
    return sorted(c for c in cols if 0 <= c < J)


@functools.lru_cache(maxsize=None)
def influence():
    """(x, y, n, m, dx, columns of m): n lies in dropped frames alone, m in kept ones; x[n] + dx leaves float64's keep mask as it is."""
    _fs, x, y, s64, _snr = reference()[0]["silent middle third"]
    kept = np.nonzero(s64.keep)[0]
    n, m, dx = 10000, 2624, np.float32(1e-3)
    for s in (n, m):
        assert s // R.HOP - 1 >= 0 and s // R.HOP < s64.K0             # two candidate frames cover the sample
    assert not s64.keep[n // R.HOP - 1] and not s64.keep[n // R.HOP]
    assert s64.keep[m // R.HOP - 1] and s64.keep[m // R.HOP]
    assert _columns(kept, s64.K - 1, n) == []
    cols = _columns(kept, s64.K - 1, m)
    assert 1 <= len(cols) <= 3
    x2 = x.copy()
    x2[n] += dx
    t64 = R.stages(x2.astype(np.float64), y.astype(np.float64), FS)
    assert np.array_equal(t64.keep, s64.keep) and R.keep_margin(t64) >= 1e-3
    t32 = R.stages(x2, y, FS, np.float32)
    assert np.array_equal(t32.keep, s64.keep)
    return x, y, n, m, dx, cols


def test_what_a_sample_may_move(ref):
    x, y, n, m, dx, cols = influence()
    yn, ym, xn = y.copy(), y.copy(), x.copy()
    yn[n] += np.float32(0.25)
    ym[m] += np.float32(0.25)
    xn[n] += dx
    clips, d, e = _both([x, x, x, xn], [y, yn, ym, y], FS)
    base = clips[0]
    _against_float64(ref, ["silent middle third"], (clips[:1], d[:1], e[:1]))
    assert base.K - 1 > max(cols)
    # a sample of the processed signal, and one of the clean signal, that only dropped frames hold
    for i in (1, 3):
        assert d[i].tobytes() == d[0].tobytes() and e[i].tobytes() == e[0].tobytes(), i
        assert np.array_equal(clips[i].keep, base.keep)
        assert _same_bits(clips[i].X, base.X) and _same_bits(clips[i].Y, base.Y), i
    # a sample of the processed signal in kept frames
    assert d[2] != d[0] and e[2] != e[0]
    assert np.array_equal(clips[2].keep, base.keep) and _same_bits(clips[2].X, base.X)
    moved = (clips[2].Y != base.Y).any(axis=0)
    assert np.nonzero(moved)[0].tolist() == cols, (np.nonzero(moved)[0].tolist(), cols)
    others = np.ones(base.Y.shape[1], bool)
    others[cols] = False
    assert _same_bits(clips[2].Y[:, others], base.Y[:, others])


# ------------------------------------------------------------------------------------------------ gain
@functools.lru_cache(maxsize=None)
def gain_pairs():
    """{rate: (x, y, [(g, g x, g y), (g, x, g y) per gain])}; the fp32 stand-in is gain-invariant on them bit for bit (so that a failure
    points at the kernel), and float32 holds g x exactly."""
    out = {}
    for fs in (FS, 24000):
        _fs, x, y, _s64, _snr = reference()[0][f"3 s at {fs} Hz"]
        s = R.stages(x, y, fs, np.float32)
        variants = []
        for g in GAINS:
            g32 = np.float32(g)
            gx, gy = x * g32, y * g32
            assert np.array_equal(gx.astype(np.float64), x.astype(np.float64) * g) and np.array_equal(gy.astype(np.float64), y.astype(np.float64) * g)
            for a, b in ((gx, gy), (x, gy)):
                t = R.stages(a, b, fs, np.float32)
                assert np.array_equal(t.keep, s.keep), (fs, g)
                assert np.float32(t.d[False]).tobytes() == np.float32(s.d[False]).tobytes(), (fs, g)
                assert np.float32(t.d[True]).tobytes() == np.float32(s.d[True]).tobytes(), (fs, g)
                variants.append((g32, a, b))
        out[fs] = (x, y, variants)
    return out


@pytest.mark.parametrize("fs", (FS, 24000))
def test_power_of_two_gain_moves_no_bit(ref, fs):
    x, y, variants = gain_pairs()[fs]
    clips, d, e = _both([x] + [v[1] for v in variants], [y] + [v[2] for v in variants], fs)
    _against_float64(ref, [f"3 s at {fs} Hz"], (clips[:1], d[:1], e[:1]))
    for i, (g, a, _b) in enumerate(variants, start=1):
        assert d[i].tobytes() == d[0].tobytes() and e[i].tobytes() == e[0].tobytes(), (fs, float(g), i, d[i], d[0], e[i], e[0])
        assert np.array_equal(clips[i].keep, clips[0].keep) and clips[i].K == clips[0].K, (fs, float(g))
        if fs != FS:
            gx = g if a is not x else np.float32(1.0)
            assert _same_bits(clips[i].xr, clips[0].xr * gx) and _same_bits(clips[i].yr, clips[0].yr * g), (fs, float(g))
