"""The loudness-range kernel alone, through the C ABI (csrc/r128.hip: wt_loudness_range), against the float64 definitions of
tests/r128_ref.py (short-term loudness, EBU Tech 3341; loudness range, EBU Tech 3342).

Tolerances: every short-term value within loudness_ref.bound of float64 (the error of the same definition through a sequential
fp32 lfilter, at least two fp32 ulps); the low and the high value within their own such bounds; LRA within the sum of the two plus
one fp32 ulp of itself (it is rounded once more); the count through the range gates equal; out[0..3) and the momentary series
the bits of wt_loudness on the same clip.  In the float64 reference no short-term value of any clip lies within 10^-3 LU of either
range gate (asserted: the seeds were chosen so), so the gated sets agree and the selected ranks are the same windows.

Lengths: at 24 kHz 71999 (no window), 72000, 72001, 74399 (one), 74400 (two); at 11025 Hz 33074 (none) and 33075 (one); at 8 kHz
24000 + 800 (k - 1), k windows, for k = 1, 2, 10, 11, 12, 20, 21, 22 (the ranks move at m = 6, 11, 16, 21, ...), one of them with
two channels; one 8 kHz clip of 110 s (S = 1071: more than four windows per thread) with a stretch under -70 LUFS and a stretch
more than 20 LU under the rest.  Noise at stepped levels, so that the range is several LU.  Every clip is measured in one batch
per rate, alone, and in a batch of more than 64 (the descriptors then travel through the workspace).
Observed errors on an MI355X: profiles/r128_error.txt."""
import math

import numpy as np
import pytest
import torch

from tests import loudness_ref as R
from tests import r128_ref as Q

pytestmark = pytest.mark.gpu

LEVELS = (-20.0, -26.0, -23.0, -31.0, -21.0, -28.0)
STAIRS = (-46.0, -34.0, -22.0, -14.0)


def _cases():
    """(name, rate, clip)"""
    out = []
    for j, n in enumerate((71999, 72000, 72001, 74399, 74400)):
        out.append(("n%d" % n, 24000, Q.make_stepped(n, 24000, 9100 + j, LEVELS, 0.5)))
    for j, n in enumerate((33074, 33075)):
        out.append(("n%d" % n, 11025, Q.make_stepped(n, 11025, 9200 + j, LEVELS, 0.5)))
    for j, k in enumerate((1, 2, 10, 11, 12, 20, 21, 22)):
        n = 24000 + 800 * (k - 1)
        step = n / 8000.0 / len(STAIRS) + 1e-3                             # one pass up the stairs: the windows differ by several LU
        x = Q.make_stepped(n, 8000, 9300 + j, STAIRS, step)
        if k == 12:
            x = np.stack([x, Q.make_stepped(n, 8000, 9350 + j, STAIRS, 0.8 * step)])
        out.append(("k%d" % k, 8000, x))
    # 110 s: 2 s steps through the levels, with 12 s at -110 dB (under -70 LUFS) and 12 s at -62 dB (more than 20 LU under the rest)
    x = Q.make_stepped(880000, 8000, 9400, LEVELS, 2.0)
    rng = np.random.default_rng(9401)
    x[30 * 8000:42 * 8000] = (rng.standard_normal(12 * 8000) * 10.0 ** (-110.0 / 20.0)).astype(np.float32)
    x[70 * 8000:82 * 8000] = (rng.standard_normal(12 * 8000) * 10.0 ** (-62.0 / 20.0)).astype(np.float32)
    out.append(("long", 8000, x))
    return out


class Case:
    def __init__(self, name, fs, x):
        self.name, self.fs, self.x = name, fs, x
        self.n = x.shape[-1]
        self.z, self.s = Q.short_term(x, fs)                               # float64
        self.z32, self.s32 = Q.short_term(x, fs, np.float32)               # the evaluation the bounds come from
        self.lra, self.lo, self.hi, self.m, self.rel, self.margin = Q.loudness_range(self.z)
        self.lra32, self.lo32, self.hi32, self.m32, _rel, _margin = Q.loudness_range(self.z32)


@pytest.fixture(scope="module")
def cases():
    """Every clip on the CPU with its float64 and fp32 references, computed once and left unchanged."""
    return [Case(*c) for c in _cases()]


@pytest.fixture(scope="module")
def measured(cases):
    """Per case {"batch", "alone", "b70"}: ((9,), l_j, s_j) each, and "loudness": wt_loudness's ((3,), l_j)."""
    got = [dict() for _ in cases]
    for fs in sorted({c.fs for c in cases}):
        idx = [j for j, c in enumerate(cases) if c.fs == fs]
        on_gpu = [torch.from_numpy(cases[j].x).cuda() for j in idx]
        out, mom, sht = Q.measure_range(on_gpu, fs)
        lout, lblocks = R.measure(on_gpu, fs)
        for r, j in enumerate(idx):
            got[j]["batch"] = (out[r], mom[r], sht[r])
            got[j]["loudness"] = (lout[r], lblocks[r])
            o1, m1, s1 = Q.measure_range([on_gpu[r]], fs)
            got[j]["alone"] = (o1[0], m1[0], s1[0])
        short = [r for r, j in enumerate(idx) if cases[j].n <= 100000]
        order = [short[k % len(short)] for k in range(66)] + list(range(len(idx)))     # 66 and more: through the workspace
        out, mom, sht = Q.measure_range([on_gpu[r] for r in order], fs)
        for pos, r in enumerate(order):
            mine = (out[pos], mom[pos], sht[pos])
            prev = got[idx[r]].setdefault("b70", mine)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(prev, mine)), (cases[idx[r]].name, "two places of one batch")
        # the series are optional: without them the nine values are the same
        out0, _m, _s = Q.measure_range(on_gpu, fs, series=False)
        for r, j in enumerate(idx):
            assert out0[r].tobytes() == got[j]["batch"][0].tobytes(), (cases[j].name, "series=False")
    return got


def test_no_short_term_value_lies_near_a_range_gate(cases):
    for c in cases:
        assert c.margin >= 1e-3, (c.name, c.margin)
        assert c.m == c.m32, c.name                                        # (the fp32 evaluation gates alike)
    long = cases[-1]
    assert len(long.s) == 1071 and long.m < int((long.s > -70.0).sum()) < 1071   # both range gates remove windows of the long clip
    assert sum(1 for c in cases if c.m > 0 and c.lra > 3.0) >= 6           # several LU where there are windows enough


def test_short_term_values_within_the_bound(cases, measured):
    from wavtokenizer_amd import _capi
    for c, g in zip(cases, measured):
        out, _mom, sht = g["batch"]
        assert len(sht) == len(c.s) == int(_capi.lib.wt_short_term_blocks(c.n, c.fs)), c.name
        worst = 0.0
        for j, (got, want, f32) in enumerate(zip(sht, c.s, c.s32)):
            err = abs(float(got) - want)
            assert err <= R.bound(want, f32), (c.name, j, err, R.bound(want, f32))
            worst = max(worst, err)
        print(f"range_error {c.name:7s} fs {c.fs:6d} n {c.n:7d} ch {c.x.ndim}  S {len(sht):5d}  short-term worst err {worst:.3e}")
        if len(sht):
            assert out[8].tobytes() == sht.max().tobytes(), c.name
        else:
            assert out[8] == -np.inf, c.name


def test_range_low_high_and_count(cases, measured):
    for c, g in zip(cases, measured):
        out = g["batch"][0]
        assert int(out[6]) == c.m, (c.name, out[6], c.m)
        if c.m == 0:
            assert np.isnan(out[3]) and np.isnan(out[4]) and np.isnan(out[5]) and out[6] == 0, c.name
            continue
        b_lo, b_hi = R.bound(c.lo, c.lo32), R.bound(c.hi, c.hi32)
        print(f"range_error {c.name:7s} fs {c.fs:6d}  LRA {float(out[3]):9.5f} LU  err {abs(float(out[3]) - c.lra):.3e}  "
              f"bound {b_lo + b_hi + R.ulp32(c.lra):.3e}  low {float(out[4]):9.4f} err {abs(float(out[4]) - c.lo):.3e}  "
              f"high {float(out[5]):9.4f} err {abs(float(out[5]) - c.hi):.3e}  m {int(out[6])}  margin {c.margin:.2e}")
        assert abs(float(out[4]) - c.lo) <= b_lo, (c.name, out[4], c.lo)
        assert abs(float(out[5]) - c.hi) <= b_hi, (c.name, out[5], c.hi)
        assert abs(float(out[3]) - c.lra) <= b_lo + b_hi + R.ulp32(c.lra), (c.name, out[3], c.lra)


def test_clips_under_three_seconds_have_no_range(cases, measured):
    seen = 0
    for c, g in zip(cases, measured):
        if c.n * 10 < 30 * c.fs:
            seen += 1
            out, mom, sht = g["batch"]
            assert np.isnan(out[3]) and np.isnan(out[4]) and np.isnan(out[5]) and out[6] == 0 and out[8] == -np.inf and len(sht) == 0, c.name
            assert np.isfinite(out[0]) and np.isfinite(out[7]) and len(mom) > 0, c.name       # (they do have a loudness)
    assert seen == 2


def test_integrated_triple_and_momentary_series_have_the_bits_of_wt_loudness(cases, measured):
    for c, g in zip(cases, measured):
        out, mom, _sht = g["batch"]
        lout, lblocks = g["loudness"]
        assert out[:3].tobytes() == lout.tobytes(), (c.name, out[:3], lout)
        assert mom.tobytes() == lblocks.tobytes(), c.name
        assert out[7].tobytes() == mom.max().tobytes(), c.name


def test_same_bits_alone_in_a_batch_and_across_the_descriptor_boundary(cases, measured):
    for c, g in zip(cases, measured):
        for key in ("alone", "b70"):
            for a, b in zip(g[key], g["batch"]):
                assert a.tobytes() == b.tobytes(), (c.name, key)
