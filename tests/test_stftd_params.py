"""The STFT-distance kernels (csrc/stftd.hip) over the parameters wt_stftd_create accepts, through ctypes as in
tests/test_stftd_op.py: clips in a NaN-filled arena, outputs between canaries, the float64 definition (tests/stftd_ref.py), bars from
the fp32 stand-ins run on the CPU in this test (never from the kernel).

Reached here and nowhere else: hop = n_fft, a window of one and of three samples, win_length = n_fft - 1 (no left padding), the
distance with one and with eight resolutions, with the widest transform first, with a repeated resolution and in another order, and
what holds exactly for any fp32 implementation: |log a - log b| is symmetric, an identical pair gives 0, and a gain of 2^k on the
clip is a gain of exactly 2^k on every magnitude above the floor (the power scales by 4^k, which keeps the exponent's parity under
the square root) and leaves every sc_r its bits.  Measured on an MI355X: profiles/stftd_error.txt."""
import functools

import numpy as np
import pytest

from tests import stftd_ref as R

pytestmark = pytest.mark.gpu

FLOOR32 = np.sqrt(np.float32(1e-7))                                          # fp32: a magnitude at the clamp

# (n_fft, hop, win_length, samples)
MAG_CASES = ((512, 512, 512, 3001), (512, 17, 33, 3001), (512, 512, 1, 3001), (1024, 1024, 1024, 3001), (1024, 1, 1024, 700),
             (2048, 2048, 2047, 3001), (2048, 999, 3, 3001))


@functools.lru_cache(maxsize=None)
def magnitude_reference():
    """(per case (clip, S64, norms), per n_fft the bar): 4 x the stand-in's worst r pooled over the n_fft's cases.  A window with one
    non-zero tap leaves the radix-2 stand-in no sum to round, only the sample's products with the twiddles (at most r = 1, and 0
    where the tap meets none), so a bar of its own would say little: the case is held to the pooled bar of its n_fft."""
    per, worst = {}, {}
    for case in MAG_CASES:
        n_fft, hop, win, n = case
        x = R.signal("noise", n, seed=11)
        S64, norms = R.magnitude64(x, n_fft, hop, win)
        r = R.error_stat(R.standin_magnitude_fp32(x, n_fft, hop, win), S64, norms)
        print(f"stftd stand-in (fp32 radix-2, CPU) n_fft {n_fft} hop {hop} win {win}: r {r:.3f}")
        worst[n_fft] = max(worst.get(n_fft, 0.0), r)
        per[case] = (x, S64, norms)
    for n_fft, w in worst.items():
        assert 1.0 < w < 4.0, (n_fft, w)                             # (the yardstick itself, as in test_stftd_op.test_other_resolutions' cases)
    return per, {n_fft: 4.0 * w for n_fft, w in worst.items()}


@pytest.mark.parametrize("case", MAG_CASES, ids=lambda c: "-".join(map(str, c)))
def test_magnitudes_at_the_edges_of_hop_and_window(case):
    per, bars = magnitude_reference()
    n_fft, hop, win, n = case
    x, S64, norms = per[case]
    (S,), ok = R.run_magnitude([x], n_fft, hop, win)
    assert ok and S.shape == S64.shape == (n_fft // 2 + 1, 1 + n // hop) and not np.isnan(S).any()
    r = R.error_stat(S, S64, norms)
    print(f"stftd_error n_fft {n_fft:4d} hop {hop} win {win} T {n}  r {r:.3f}  (bar {bars[n_fft]:.3f})")
    assert r <= bars[n_fft]
    if win == 1:                                                    # |x[n]| in every bin, and not the floor an all-zero window would give
        assert bool((S64 > 10 * FLOOR32).any()) and float(np.abs(S64 - S64[:1]).max()) < 1e-12


DEFAULT = tuple(R.RESOLUTIONS)
EIGHT = ((512, 50, 240), (2048, 240, 1200)) * 4
SETS = {"one narrow window": ((512, 512, 3),),
        "one widest, no left padding": ((2048, 2048, 2047),),
        "mixed edges": ((1024, 1024, 1024), (512, 17, 33), (2048, 999, 3)),
        "default reversed": DEFAULT[::-1],
        "eight": EIGHT}


@functools.lru_cache(maxsize=None)
def distance_reference():
    """(estimate, target, per set (float64 total, components), bar)."""
    y = R.signal("noise", 3001, seed=3)
    x = R.estimate_of("noise", y)
    per, worst = {}, 0.0
    for name, res in SETS.items():
        d64, c64 = R.distance64(x, y, res)
        d32, c32 = R.standin_distance_fp32(x, y, res)
        worst = max(worst, abs(d32 - d64) / d64, float((np.abs(c32 - c64) / c64).max()))
        per[name] = (d64, c64)
    bar = min(4.0 * worst, 1e-5)
    print(f"stftd distance stand-in (torch.stft fp32, CPU) over the resolution sets: worst relative error {worst:.3e}, bar {bar:.3e}")
    assert 1e-8 < worst < 1e-5
    return x, y, per, bar


@pytest.fixture(scope="module")
def distances():
    """One call per resolution set, and the default set, on the one pair."""
    x, y, _per, _bar = distance_reference()
    got, intact = {}, True
    for name, res in list(SETS.items()) + [("default", DEFAULT)]:
        (got[name],), ok = R.run_distance([x], [y], res)
        intact = intact and ok
    return got, intact


@pytest.mark.parametrize("name", list(SETS))
def test_distance_against_float64_per_resolution_set(distances, name):
    _x, _y, per, bar = distance_reference()
    got, intact = distances
    g = got[name]
    d64, c64 = per[name]
    n_res = len(SETS[name])
    assert intact and g.shape == (1 + 2 * n_res,) and np.isfinite(g).all()
    comps = g[1:].reshape(-1, 2)
    rel = max(abs(float(g[0]) - d64) / d64, float((np.abs(comps.astype(np.float64) - c64) / c64).max()))
    print(f"stftd_distance {name:28s} n_res {n_res}  d {float(g[0]):.7f}  float64 {d64:.7f}  worst relative error {rel:.3e}  (bar {bar:.3e})")
    assert g[0] == R.total_fp32(comps)                               # the components add up to the total as defined
    assert rel <= bar


def test_a_repeated_resolution_repeats_its_bits(distances):
    got, _intact = distances
    comps = got["eight"][1:].reshape(8, 2)
    for r in range(2, 8):
        assert np.array_equal(comps[r], comps[r % 2]), (r, comps)
    assert not np.array_equal(comps[0], comps[1])


def test_the_order_of_the_resolutions_moves_only_the_total(distances):
    got, _intact = distances
    fwd, rev = got["default"][1:].reshape(3, 2), got["default reversed"][1:].reshape(3, 2)
    assert np.array_equal(rev, fwd[::-1]), (fwd, rev)
    assert got["default"][0] == R.total_fp32(fwd) and got["default reversed"][0] == R.total_fp32(rev)
    assert len({tuple(c) for c in fwd}) == 3                         # (three different resolutions: a swapped table would show)


def test_eight_resolutions_in_a_call_of_65_pairs(distances):
    """Descriptors through the workspace, eight blocks of partials per pair, mixed lengths: the pair at both ends has the bits it
    has alone."""
    x, y, _per, _bar = distance_reference()
    got, _intact = distances
    lengths = (1025, 1500, 2047, 4100)
    est, tgt = [], []
    for i in range(65):
        t = R.signal("noise", lengths[i % 4], seed=20 + i)
        tgt.append(t)
        est.append(R.estimate_of("noise", t))
    for pos in (0, 64):
        est[pos], tgt[pos] = x, y
    many, ok = R.run_distance(est, tgt, EIGHT)
    assert ok and not any(np.isnan(g).any() for g in many)
    for pos in (0, 64):
        assert np.array_equal(many[pos], got["eight"]), pos
    (one,), ok = R.run_distance([est[63]], [tgt[63]], EIGHT)          # and a neighbour of the last, 4100 samples
    assert ok and np.array_equal(many[63], one)


def test_swap_symmetry_and_an_identical_pair(distances):
    x, y, _per, _bar = distance_reference()
    got, _intact = distances
    (swapped,), ok = R.run_distance([y], [x])
    assert ok
    assert np.array_equal(swapped[2::2], got["default"][2::2])        # mag_r: |log a - log b|, the same order of summation
    assert not np.array_equal(swapped[1::2], got["default"][1::2])    # (sc_r divides by the target's norm: the pair is not symmetric)
    (same,), ok = R.run_distance([y], [y])
    assert ok and same.shape == (7,) and bool((same == 0.0).all())
    assert float(np.abs(y).max()) > 0.1


MAG_GAINS = (2.0 ** 2, 2.0 ** 7)


def test_a_power_of_two_gain_scales_the_magnitudes_and_keeps_sc(distances):
    x, y, _per, _bar = distance_reference()
    got, _intact = distances
    scaled = [[(np.float32(g) * s).astype(np.float32) for s in (x, y)] for g in MAG_GAINS]
    for n_fft, hop, win in DEFAULT:
        S, ok = R.run_magnitude([x, y] + [s for pair in scaled for s in pair], n_fft, hop, win)
        assert ok
        # the condition of the sc_r claim below: no bin of either signal at the clamp (the smallest float64 magnitude of this pair is
        # 6.8e-4 against 3.2e-4)
        assert float(S[0].min()) > FLOOR32 and float(S[1].min()) > FLOOR32, (n_fft, S[0].min(), S[1].min())
        for i, g in enumerate(MAG_GAINS):
            for j in (0, 1):
                assert np.array_equal(S[2 + 2 * i + j], np.float32(g) * S[j]), (n_fft, g, j)        # bit for bit
    for g, (gx, gy) in zip(MAG_GAINS, scaled):
        (gd,), ok = R.run_distance([gx], [gy])
        assert ok and np.array_equal(gd[1::2], got["default"][1::2]), (g, gd, got["default"])
