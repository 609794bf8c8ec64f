"""The STOI kernels (csrc/stoi.hip) at the rates tests/test_stoi_op.py does not launch, stage by stage against the float64
definition (tests/stoi_ref.py), with that module's statistics and rules:
     8000 Hz  p / q = 5 / 4: the one rate that upsamples; at the right edge the first taps meet input samples past the last one
    11025 Hz  p = 400 of the phase table's 448 entries; the filter does not fit LDS (stoi_resample_kernel)
    22050 Hz  p = 200; stoi_resample_kernel
    32000 Hz, 48000 Hz  the longest filters of stoi_resample_lds_kernel
Per rate: the longest clip with K0 = 30 (1e-5, and the resampler's right edge), one sample more (K0 = 31: one segment) and about
1 s whose length at 10 kHz is no multiple of 256 (the last resampler block is partial); at 8000 and 22050 Hz also a clip with a
silent middle third, so that both resampler paths feed a kept-frame list with a gap.  A rate's cases go in one call per measure;
the 1 s clip is also launched alone and must have the bits of its place in the batch.

The bars are 4 x the worst deviation the fp32 stand-in reaches over this module's cases, computed on the CPU here, never from the
kernel.  Measured on an MI355X: profiles/stoi_error.txt."""
import functools

import numpy as np
import pytest

from tests import stoi_ref as R
from tests.test_stoi_op import _deviations, _shaped

pytestmark = pytest.mark.gpu

# rate: the longest clip with K0 = 30, the shortest with K0 = 31, about 1 s
LENGTHS = {8000: (3276, 3277, 8137), 11025: (4515, 4516, 11162), 22050: (9031, 9032, 22187), 32000: (13107, 13108, 32137),
           48000: (19660, 19661, 48137)}
RATES = tuple(LENGTHS)
SNRS = (20, 0, -10)
SEEDS = (20, 21, 22)
GAPPED = (8000, 22050)


def _cases():
    """(name, rate, samples, shape, SNR in dB, seed)"""
    out = []
    for fs, (t30, t31, t1s) in LENGTHS.items():
        out.append((f"{fs} Hz, K0 = 30: the 1e-5 path", fs, t30, None, SNRS[0], SEEDS[0]))
        out.append((f"{fs} Hz, K0 = 31: one segment", fs, t31, None, SNRS[1], SEEDS[1]))
        out.append((f"{fs} Hz, 1 s", fs, t1s, None, SNRS[2], SEEDS[2]))
        if fs in GAPPED:
            out.append((f"{fs} Hz, silent middle third", fs, 2 * fs + 137, "middle", SNRS[0], 23))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def reference():
    """Per case: the pair and the float64 stages, the conditions asserted; the four bars.  CPU only."""
    out = {}
    worst = dict(res=0.0, band=0.0, d=0.0, e=0.0)
    for name, fs, T, shape, snr, seed in CASES:
        x = _shaped(T, fs, seed, shape)
        y = R.noisy(x, snr, seed=seed)
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
    for fs in RATES:
        assert (out[f"{fs} Hz, K0 = 30: the 1e-5 path"][2].K0, out[f"{fs} Hz, K0 = 30: the 1e-5 path"][2].K) == (30, 30), fs
        assert out[f"{fs} Hz, K0 = 30: the 1e-5 path"][2].d[False] == R.SHORT
        assert (out[f"{fs} Hz, K0 = 31: one segment"][2].K0, out[f"{fs} Hz, K0 = 31: one segment"][2].K) == (31, 31), fs
        s = out[f"{fs} Hz, 1 s"][2]
        assert 70 <= s.K0 == s.K <= 80 and R.resampled_length(LENGTHS[fs][2], fs) % 256, fs
    for fs in GAPPED:
        s = out[f"{fs} Hz, silent middle third"][2]
        assert 31 < s.K < s.K0 - 20 and np.diff(np.nonzero(s.keep)[0]).max() > 20, fs
    # the rates as the header describes them: one that upsamples, two on the global-memory resampler with p = 200 and 400
    assert R.ratio(8000) == (5, 4) and R.ratio(22050)[0] == 200 and R.ratio(11025)[0] == 400
    bars = {k: 4.0 * v for k, v in worst.items()}
    print("stoi_error stand-in (fp32, sequential sums, radix-2 FFT, CPU) over tests/test_stoi_rates.py: worst resampled %.3e  bands %.3e  "
          "STOI %.3e  ESTOI %.3e; the bars are 4 x these" % (worst["res"], worst["band"], worst["d"], worst["e"]))
    # (the yardstick itself: fp32 rounding, not a broken stand-in)
    assert 1e-8 < worst["res"] < 1e-5 and 1e-8 < worst["band"] < 1e-4 and 0 < worst["d"] < 1e-4 and 0 < worst["e"] < 1e-4
    return out, bars


@pytest.fixture(scope="module")
def ref():
    return reference()


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
    for name, fs, T, _shape, snr, _seed in CASES:
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


@pytest.mark.parametrize("fs", RATES)
def test_the_one_second_clip_alone_has_the_bits_of_its_place_in_the_batch(ref, launched, fs):
    cases, _bars = ref
    got, _ = launched
    name = f"{fs} Hz, 1 s"
    x, y, _s64 = cases[name]
    s, d, e = got[name]
    plain = R.run([x], [y], fs, extended=False)
    ext = R.run([x], [y], fs, extended=True, with_taps=False)
    assert plain.intact and ext.intact
    assert plain.d[0].tobytes() == d.tobytes() and ext.d[0].tobytes() == e.tobytes()
    for f in ("xr", "yr", "keep", "X", "Y"):
        assert np.array_equal(getattr(plain.clips[0], f), getattr(s, f)), f
