"""The mel kernels (csrc/mel.hip) over the parameters wt_mel_create accepts, through ctypes as in tests/test_mel_op.py: clips in a
NaN-filled arena, outputs between canaries, the float64 definition (tests/mel_ref.py), bars from the fp32 radix-2 stand-in run on the
CPU in this test (never from the kernel).

Reached here and nowhere else: the second filter of a lane (lane + 64) at n_mels 64, 65, 127 and 128 and a single filter; a filter
without a bin (44.1 and 48 kHz at 127 and 128 filters); the sparse weight table near its capacity (8 and 16 kHz, 127 and 128
filters); hop_length 1, an odd one and 1024; more than 64 frames in mel_mean_block; and that a gain of 2^k on the clip is a gain of
exactly 2^k on the linear mel values (every product and sum of the chain scales without a rounding of its own; the power scales by
4^k, which keeps the exponent's parity under the square root).  Measured on an MI355X: profiles/mel_error.txt."""
import functools

import numpy as np
import pytest

from tests import mel_ref as R

pytestmark = pytest.mark.gpu

RATES = (8000, 16000, 22050, 24000, 44100, 48000)
MELS = (1, 2, 63, 64, 65, 100, 127, 128)
GRID = [(sr, m) for sr in RATES for m in MELS]
ONE_EMPTY = {(44100, 127), (44100, 128), (48000, 127), (48000, 128)}          # (asserted below from the tables, not taken from the kernel)
HOP, T = 256, 3000
LOG_FLOOR = np.log(np.float32(1e-7))                                        # fp32: what test_mel_op.test_frames_of_zeros pins


@functools.lru_cache(maxsize=None)
def grid_reference():
    """(clip, per pair (M64, norms), bar): the grid of (sample_rate, n_mels) at hop 256 on one clip of noise."""
    x = R.signal("noise", T)
    per, rs = {}, []
    for sr, m in GRID:
        M64, norms = R.mel64(x, sr, HOP, m)
        rs.append(R.error_stat(R.standin_fp32(x, sr, HOP, m), M64, norms, sr, m))
        per[(sr, m)] = (M64, norms)
    print(f"mel stand-in (fp32 radix-2, CPU) over the (rate, n_mels) grid: worst r {max(rs):.3f}, smallest {min(rs):.3f}, bar {4 * max(rs):.3f}")
    # (the yardstick itself; the worst is the single filter over all 513 bins: 513 rounded sums in a row)
    assert 0.5 < max(rs) < 8.0
    return x, per, 4.0 * max(rs)


@pytest.fixture(scope="module")
def grid():
    return grid_reference()


@pytest.fixture(scope="module")
def grid_launched(grid):
    """Per pair one handle and one launch in linear mode, one more in log mode."""
    x = grid[0]
    lin, log, intact = {}, {}, True
    for sr, m in GRID:
        (lin[(sr, m)],), ok1 = R.run([x], log=False, sample_rate=sr, hop=HOP, n_mels=m)
        (log[(sr, m)],), ok2 = R.run([x], log=True, sample_rate=sr, hop=HOP, n_mels=m)
        intact = intact and ok1 and ok2
    return lin, log, intact


def test_the_grid_has_one_empty_filter_at_four_pairs():
    """(the definition's own property, on the CPU: what the GPU rows are compared with below)"""
    assert {p for p in GRID if len(R.empty_filters(*p)) == 1} == ONE_EMPTY
    assert all(len(R.empty_filters(*p)) == 0 for p in GRID if p not in ONE_EMPTY)


def test_linear_mel_against_float64_over_rates_and_filter_counts(grid, grid_launched):
    _x, per, bar = grid
    lin, _log, intact = grid_launched
    assert intact
    bad = []
    for p in GRID:
        M64, norms = per[p]
        assert lin[p].shape == M64.shape == (p[1], 1 + T // HOP) and not np.isnan(lin[p]).any(), p
        r = R.error_stat(lin[p], M64, norms, *p)                      # (asserts exact zeros where the scale is zero: the empty filters)
        print(f"mel_error noise      T {T:5d} F {M64.shape[1]:3d}  r {r:.3f}  (bar {bar:.3f}; {p[0]} Hz, hop {HOP}, {p[1]} mels)")
        if not r <= bar:
            bad.append((p, r))
        zero_rows = np.nonzero((lin[p] == 0).all(axis=1))[0]
        assert np.array_equal(zero_rows, R.empty_filters(*p)), (p, zero_rows)
        assert len(zero_rows) == (1 if p in ONE_EMPTY else 0), p
    assert not bad, bad


def test_log_mel_against_float64_over_rates_and_filter_counts(grid, grid_launched):
    """No entry is left out of the bound at any pair: with this clip the float64 reference alone keeps b < M64 / 2 everywhere (the
    smallest margin is printed), and an empty filter's row has b = 0 and is held to the 2 ulp of the clipped constant."""
    _x, per, bar = grid
    _lin, log, intact = grid_launched
    assert intact
    for p in GRID:
        M64, norms = per[p]
        bound, skip = R.log_bound(bar, M64, norms, *p)
        assert int(skip.sum()) == 0, (p, int(skip.sum()))
        err = np.abs(log[p].astype(np.float64) - R.safe_log(M64))
        worst = float((err / bound).max())
        print(f"mel_log_error noise      T {T:5d}  max err / bound {worst:.3f}  ({p[0]} Hz, hop {HOP}, {p[1]} mels)")
        assert bool((err <= bound).all()), (p, worst)
        for row in R.empty_filters(*p):
            vals = np.unique(log[p][row])
            assert vals.shape == (1,) and abs(float(vals[0]) - float(LOG_FLOOR)) <= float(np.spacing(np.abs(LOG_FLOOR))), (p, row, vals)


HOPS = ((1, 700), (255, 3000), (1024, 3000))                                 # (hop, samples): 701, 12 and 3 frames


@functools.lru_cache(maxsize=None)
def hops_reference():
    per, rs = {}, []
    for hop, n in HOPS:
        x = R.signal("noise", n)
        M64, norms = R.mel64(x, 24000, hop, 100)
        rs.append(R.error_stat(R.standin_fp32(x, 24000, hop, 100), M64, norms))
        per[hop] = (x, M64, norms)
    print("mel stand-in (fp32 radix-2, CPU) at hop " + ", ".join(f"{h}: r {r:.3f}" for (h, _n), r in zip(HOPS, rs)) + f"; bar {4 * max(rs):.3f}")
    assert 0.5 < max(rs) < 8.0
    return per, 4.0 * max(rs)


def test_hop_lengths_one_odd_and_n_fft():
    """Above 512 the frames no longer cover every sample; at 1 consecutive frames differ by one sample."""
    per, bar = hops_reference()
    for hop, n in HOPS:
        x, M64, norms = per[hop]
        (M,), ok = R.run([x], log=False, hop=hop)
        assert ok and M.shape == M64.shape == (100, 1 + n // hop) and not np.isnan(M).any(), hop
        r = R.error_stat(M, M64, norms)
        print(f"mel_error noise      T {n:5d} F {M.shape[1]:3d}  r {r:.3f}  (bar {bar:.3f}; 24000 Hz, hop {hop}, 100 mels)")
        assert r <= bar, (hop, r)


LONG = ((64, 6300), (65, 6400), (128, 12700), (129, 12800), (200, 19900))   # (frames, samples) at hop 100
PLACES = (0, 17, 35, 52, 69)


@functools.lru_cache(maxsize=None)
def long_reference():
    """Per clip length the pair, both sides' (M64, norms) and the bar: 4 x the stand-in's worst r over the ten clips."""
    per, worst = {}, 0.0
    for F, n in LONG:
        a, b = R.noisy_pair(n)
        sides = []
        for s in (a, b):
            M64, norms = R.mel64(s, 24000, 100, 100)
            assert M64.shape == (100, F)
            worst = max(worst, R.error_stat(R.standin_fp32(s, 24000, 100, 100), M64, norms))
            sides.append((M64, norms))
        per[n] = (a, b, sides)
    print(f"mel stand-in (fp32 radix-2, CPU) on the long pairs at hop 100: worst r {worst:.3f}, bar {4 * worst:.3f}")
    assert 0.5 < worst < 8.0
    return per, 4.0 * worst


def test_distance_of_clips_of_more_than_64_frames():
    """mel_mean_block's second to fourth trip of the lane loop, and partials past index 63 of a clip: F = 64, 65, 128, 129 and 200."""
    per, bar = long_reference()
    kw = dict(hop=100)
    a = [per[n][0] for _F, n in LONG]
    b = [per[n][1] for _F, n in LONG]
    La, ok_a = R.run(a, **kw)
    Lb, ok_b = R.run(b, **kw)
    assert ok_a and ok_b
    alone = []
    for i, (F, n) in enumerate(LONG):
        (d,), ok = R.run([a[i]], [b[i]], **kw)
        assert ok and La[i].shape == (100, F)
        assert d == R.distance_fp32(La[i], Lb[i]), (F, d)              # the bits of the kernels' own summation order
        # float64, as test_mel_op.test_distance_against_its_own_spectrogram_and_against_float64 derives it: the mean of the two
        # sides' log bounds
        (Ma, na), (Mb, nb) = per[n][2]
        ba, sa = R.log_bound(bar, Ma, na)
        bb, sb = R.log_bound(bar, Mb, nb)
        assert not sa.any() and not sb.any()
        d64 = float(np.abs(R.safe_log(Ma) - R.safe_log(Mb)).mean())
        tol = float((ba + bb).mean())
        print(f"mel_distance noise / noisy copy T {n:5d} F {F:3d}  d {float(d):.6f}  float64 {d64:.6f}  |diff| {abs(float(d) - d64):.2e}  tol {tol:.2e}")
        assert abs(float(d) - d64) <= tol, (F, d, d64)
        alone.append(d)
    filler = R.signal("noise", 600, seed=5)
    many_a, many_b = [filler] * 70, [filler[::-1].copy()] * 70
    for i, at in enumerate(PLACES):
        many_a[at], many_b[at] = a[i], b[i]
    for fill in (0xAB, 0x00):
        got, ok = R.run(many_a, many_b, ws_fill=fill, **kw)           # 70 pairs: descriptors through the workspace
        assert ok and not np.isnan(got).any()
        for i, at in enumerate(PLACES):
            assert got[at] == alone[i], (fill, at, got[at], alone[i])
        assert got[1] == got[68] and got[1] > 0


GAINS = (2.0 ** -6, 2.0 ** 2, 2.0 ** 10)


@pytest.mark.parametrize("sample_rate,hop,n_mels", [(24000, 256, 100), (48000, 1024, 128)])
def test_a_power_of_two_gain_scales_the_linear_mel_exactly(sample_rate, hop, n_mels):
    kw = dict(sample_rate=sample_rate, hop=hop, n_mels=n_mels)
    x = R.signal("noise", T, seed=6)
    clips = [x] + [(np.float32(g) * x).astype(np.float32) for g in GAINS]
    for g, c in zip(GAINS, clips[1:]):
        assert np.array_equal(c.astype(np.float64), g * x.astype(np.float64))       # the gain itself rounds nothing
    lin, ok1 = R.run(clips, log=False, **kw)
    log, ok2 = R.run(clips, log=True, **kw)
    assert ok1 and ok2 and not any(np.isnan(v).any() for v in lin + log)
    empty = R.empty_filters(sample_rate, n_mels)
    assert len(empty) == (1 if (sample_rate, n_mels) in ONE_EMPTY else 0)
    live = np.ones(n_mels, bool)
    live[empty] = False
    assert float(lin[0][live].min()) * min(GAINS) > 1e-7              # noise at 0.1: no live entry reaches the clamp at any of the gains
    assert np.unique(log[0][~live]).size == len(empty)                # (the empty filter: one constant, pinned in the grid's log test)
    for g, M, L in zip(GAINS, lin[1:], log[1:]):
        assert np.array_equal(M, np.float32(g) * lin[0]), g           # bit for bit
        assert np.array_equal(L[~live], log[0][~live]), g             # at the clamp a gain moves nothing
        diff = L[live].astype(np.float64) - log[0][live].astype(np.float64) - np.log(g)
        ulp = R.ulp32(np.maximum(np.abs(L[live]), np.abs(log[0][live])))
        worst = float((np.abs(diff) / ulp).max())
        print(f"mel_gain {sample_rate} Hz hop {hop} {n_mels} mels  gain 2^{int(np.log2(g)):+d}  linear exact, log within {worst:.2f} ulp of log g")
        assert worst <= 3.0, (g, worst)
