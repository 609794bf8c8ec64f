"""The STOI kernels (csrc/stoi.hip) alone, through ctypes and the taps: pairs in a NaN-filled arena, outputs between canaries,
against the float64 definition (tests/stoi_ref.py), stage by stage: the resampled signals, the keep mask and (K0, K), the band
matrices and the final STOI and ESTOI.

The keep mask and the counts must equal float64's exactly; the cases are conditioned for that on the CPU first (every candidate
frame's norm at least 1e-3 relative away from the threshold, every centred row norm at least 1e-3 of its raw norm).  The three
fp32 comparisons each have a bar of 4 x the worst deviation an fp32 stand-in of the same chain (plain sequential sums, a radix-2
FFT, run on the CPU in this test, never the kernel) reaches over the same cases:
    resampled   max |y - y64| / max |y64| per clip
    bands       max |X - X64| / sqrt(sum_b X64[b][j]^2) per clip (an FFT's rounding is relative to the frame, not to the bin)
    d           |d - d64|, STOI and ESTOI apart
Measured on an MI355X: profiles/stoi_error.txt."""
import numpy as np
import pytest

from tests import stoi_ref as R

pytestmark = pytest.mark.gpu


def _shaped(T, fs, seed, shape):
    x = R.speechlike(T, fs, seed).astype(np.float64)
    g = np.ones(T)
    if shape == "middle":                                             # a silent middle third: the kept frames are not contiguous
        g[T // 3: 2 * T // 3] = 1e-4
    elif shape == "ends":                                             # leading and trailing silence
        g[: T // 5] = 1e-4
        g[-T // 4:] = 1e-4
    elif shape == "mostly":                                           # silence that brings J below 30
        g[2500:] = 1e-4
    return (x * g).astype(np.float32)


# (name, rate, samples, shape, SNR of the processed signal in dB)
CASES = [
    ("K0 = 30: the 1e-5 path", 10000, 4096, None, 20),
    ("J = 30: one segment", 10000, 4097, None, 0),
    ("two segments", 10000, 4225, None, -10),
    ("too short at 24 kHz", 24000, 9830, None, 0),
    ("one segment at 24 kHz", 24000, 9831, None, 20),
    ("one segment at 16 kHz", 16000, 6554, None, -10),
    ("one segment at 44.1 kHz", 44100, 18064, None, 0),
    ("3 s at 24 kHz", 24000, 72000, None, 0),
    ("3 s at 24 kHz, 20 dB", 24000, 72000, None, 20),
    ("3 s at 24 kHz, -10 dB", 24000, 72000, None, -10),
    ("silent middle third", 24000, 48000, "middle", 20),
    ("leading and trailing silence", 10000, 12000, "ends", 0),
    ("silence leaves J < 30", 10000, 6000, "mostly", 20),
    ("40 s: the select kernel's chunk loop", 10000, 400000, None, -10),
]
RATES = sorted({c[1] for c in CASES})


@pytest.fixture(scope="module")
def ref():
    """Per case: the pair, the float64 stages, the fp32 stand-in's stages; the conditions asserted; the three bars."""
    out = {}
    worst = dict(res=0.0, band=0.0, d=0.0, e=0.0)
    for i, (name, fs, T, shape, snr) in enumerate(CASES):
        x = _shaped(T, fs, i, shape)
        y = R.noisy(x, snr, seed=i)
        s64 = R.stages(x.astype(np.float64), y.astype(np.float64), fs)
        assert s64.K0 == R.candidate_frames(R.resampled_length(T, fs))
        margin = R.keep_margin(s64)
        assert margin >= 1e-3, (name, margin)
        assert min(s64.cond.values()) >= 1e-3, (name, s64.cond)
        s32 = R.stages(x, y, fs, np.float32, keep=s64.keep)
        dev = _deviations(s32, s64, fs)
        for k in worst:
            worst[k] = max(worst[k], dev[k])
        out[name] = (x, y, s64)
    # what the cases are there for
    K = {name: (out[name][2].K0, out[name][2].K) for name in out}
    assert K["K0 = 30: the 1e-5 path"] == (30, 30) and K["J = 30: one segment"] == (31, 31) and K["two segments"] == (32, 32)
    assert K["too short at 24 kHz"] == (30, 30) and K["one segment at 24 kHz"] == (31, 31)
    assert K["one segment at 16 kHz"] == (31, 31) and K["one segment at 44.1 kHz"] == (31, 31)
    k0, k = K["silent middle third"]
    assert 31 < k < k0 - 20 and np.diff(np.nonzero(out["silent middle third"][2].keep)[0]).max() > 20
    k0, k = K["leading and trailing silence"]
    keep = out["leading and trailing silence"][2].keep
    assert 31 < k < k0 and not keep[0] and not keep[-1]
    k0, k = K["silence leaves J < 30"]
    assert k0 > 31 and 1 < k < 31 and out["silence leaves J < 30"][2].d[False] == R.SHORT
    assert K["40 s: the select kernel's chunk loop"][0] > 3000
    bars = {k: 4.0 * v for k, v in worst.items()}
    print("stoi_error stand-in (fp32, sequential sums, radix-2 FFT, CPU): worst resampled %.3e  bands %.3e  STOI %.3e  ESTOI %.3e; "
          "the bars are 4 x these" % (worst["res"], worst["band"], worst["d"], worst["e"]))
    # (the yardstick itself: fp32 rounding, not a broken stand-in)
    assert 1e-8 < worst["res"] < 1e-5 and 1e-8 < worst["band"] < 1e-4 and 0 < worst["d"] < 1e-4 and 0 < worst["e"] < 1e-4
    return out, bars


def _deviations(s, s64, fs):
    """The statistics of the docstring for one clip's stages s against float64's."""
    dev = dict(res=0.0, band=0.0)
    if fs != R.FS:
        for a, b in ((s.xr, s64.xr), (s.yr, s64.yr)):
            dev["res"] = max(dev["res"], float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()))
    for a, b in ((s.X, s64.X), (s.Y, s64.Y)):
        assert a.shape == b.shape
        if b.shape[1]:
            scale = np.sqrt((b * b).sum(axis=0))
            dev["band"] = max(dev["band"], float((np.abs(a.astype(np.float64) - b) / scale[None, :]).max()))
    dev["d"] = abs(float(s.d[False]) - float(s64.d[False])) if False in s.d else 0.0
    dev["e"] = abs(float(s.d[True]) - float(s64.d[True])) if True in s.d else 0.0
    return dev


@pytest.fixture(scope="module")
def launched(ref):
    """Every case of a rate in one STOI and one ESTOI call with taps: {name: (stages from the STOI call's taps, d, e)}, intact."""
    cases, _bars = ref
    got, intact = {}, True
    for fs in RATES:
        names = [c[0] for c in CASES if c[1] == fs]
        xs, ys = [cases[n][0] for n in names], [cases[n][1] for n in names]
        plain = R.run(xs, ys, fs, extended=False)
        ext = R.run(xs, ys, fs, extended=True)
        intact = intact and plain.intact and ext.intact
        for i, n in enumerate(names):
            a, b = plain.clips[i], ext.clips[i]
            for f in ("xr", "yr", "keep", "X", "Y"):                # the stages do not depend on the measure asked for
                assert np.array_equal(getattr(a, f), getattr(b, f)), (n, f)
            assert (a.K0, a.K) == (b.K0, b.K)
            got[n] = (a, plain.d[i], ext.d[i])
    return got, intact


def test_canaries_and_no_nan(launched):
    got, intact = launched
    assert intact
    for n, (s, d, e) in got.items():
        assert np.isfinite(d) and np.isfinite(e), n
        assert not np.isnan(s.X).any() and not np.isnan(s.Y).any() and not np.isnan(s.xr).any() and not np.isnan(s.yr).any(), n


def test_keep_mask_and_counts_equal_float64(ref, launched):
    cases, _bars = ref
    got, _ = launched
    for name, (_x, _y, s64) in cases.items():
        s = got[name][0]
        assert (s.K0, s.K) == (s64.K0, s64.K), name
        assert np.array_equal(s.keep, s64.keep), name


def test_stages_against_float64(ref, launched):
    cases, bars = ref
    got, _ = launched
    bad = []
    for name, fs, T, _shape, snr in CASES:
        s64 = cases[name][2]
        s, d, e = got[name]
        s.d = {False: d, True: e}
        dev = _deviations(s, s64, fs)
        print(f"stoi_error {name:38s} {fs:5d} Hz T {T:6d} SNR {snr:3d}  K0 {s.K0:4d} K {s.K:4d}  STOI {float(d):.6f} (float64 {s64.d[False]:.6f})  "
              f"ESTOI {float(e):.6f} (float64 {s64.d[True]:.6f})  resampled {dev['res']:.2e} (bar {bars['res']:.2e})  "
              f"bands {dev['band']:.2e} (bar {bars['band']:.2e})  |d| {dev['d']:.2e} (bar {bars['d']:.2e})  |e| {dev['e']:.2e} (bar {bars['e']:.2e})")
        for k in ("res", "band", "d", "e"):
            if not dev[k] <= bars[k]:
                bad.append((name, k, dev[k], bars[k]))
        if s64.K - 1 < R.N_SEG:
            assert d == np.float32(R.SHORT) and e == np.float32(R.SHORT), name
    assert not bad, bad


def test_monotone_over_the_three_snrs(launched):
    got, _ = launched
    d = [float(got[n][1]) for n in ("3 s at 24 kHz, 20 dB", "3 s at 24 kHz", "3 s at 24 kHz, -10 dB")]
    e = [float(got[n][2]) for n in ("3 s at 24 kHz, 20 dB", "3 s at 24 kHz", "3 s at 24 kHz, -10 dB")]
    assert 1 > d[0] > d[1] > d[2] > 0 and 1 > e[0] > e[1] > e[2] > 0 and all(a != b for a, b in zip(d, e))


def test_workspace_contents_taps_and_position_do_not_matter(ref, launched):
    cases, _bars = ref
    got, _ = launched
    for fs in (10000, 24000):
        names = [c[0] for c in CASES if c[1] == fs and c[2] < 100000]
        xs, ys = [cases[n][0] for n in names], [cases[n][1] for n in names]
        for ext in (False, True):
            want = np.array([got[n][2 if ext else 1] for n in names], np.float32)
            zero = R.run(xs, ys, fs, extended=ext, ws_fill=0x00)
            nan = R.run(xs, ys, fs, extended=ext, ws_fill=0xFF)                    # (0xFFFFFFFF is a NaN)
            bare = R.run(xs[::-1], ys[::-1], fs, extended=ext, with_taps=False)
            assert zero.intact and nan.intact and bare.intact
            assert np.array_equal(zero.d, want) and np.array_equal(nan.d, want) and np.array_equal(bare.d[::-1], want), (fs, ext)
            for i, n in enumerate(names):
                for f in ("keep", "X", "Y"):
                    assert np.array_equal(getattr(zero.clips[i], f), getattr(got[n][0], f)), (n, f)
                    assert np.array_equal(getattr(nan.clips[i], f), getattr(got[n][0], f)), (n, f)
