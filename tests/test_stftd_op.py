"""The STFT-distance kernels (csrc/stftd.hip) alone, through ctypes: clips in a NaN-filled arena, outputs between canaries, against
the float64 definition (tests/stftd_ref.py) with bars that come from fp32 stand-ins run on the CPU in this test (never from the
kernel), and for what a frame, a pair and a call must not depend on.

Check 1, magnitudes per bin: r = max |S - S64| / (2^-23 (||w x_f||_2 + S64)); the bar of an n_fft is 4 x the largest r an fp32
radix-2 transform reaches over that n_fft's cases (a higher radix, the split pass of a half-length real FFT and a fast sqrt reorder
the rounding steps of a radix-2 transform but do not multiply them).
Check 2, distance values on the broadband cases: sc_r, mag_r and the total against float64, relative; the bar is 4 x the worst
relative error of torch.stft in fp32 on the CPU with fp32 sums over the same cases, and never above 1e-5.
Measured on an MI355X: profiles/stftd_error.txt."""
import numpy as np
import pytest

from tests import stftd_ref as R

pytestmark = pytest.mark.gpu

# per n_fft: n_fft / 2 + 1 (both reflections fall in one frame), k hop - 1, k hop, k hop + 1 for the smallest k that fits, and about
# 6000 samples; F = 1 + T // hop does not fill the last workgroup of four frames at (600, 120): 6, (1200, 240): 6, (300, 50): 7
LENGTHS = {1024: (513, 599, 600, 601, 6007), 2048: (1025, 1199, 1200, 1201, 6007), 512: (257, 299, 300, 301, 6007)}
RES = {n_fft: (n_fft, hop, win) for n_fft, hop, win in R.RESOLUTIONS}
CASES = {n_fft: [(name, T) for name in R.SIGNALS for T in LENGTHS[n_fft]] for n_fft in RES}


@pytest.fixture(scope="module")
def ref():
    """Per n_fft: per case the clip, S64 and the frame norms; and the bar."""
    out = {}
    for n_fft, cases in CASES.items():
        worst, per = 0.0, {}
        for name, T in cases:
            x = R.signal(name, T)
            S64, norms = R.magnitude64(x, *RES[n_fft])
            worst = max(worst, R.error_stat(R.standin_magnitude_fp32(x, *RES[n_fft]), S64, norms))
            per[(name, T)] = (x, S64, norms)
        print(f"stftd stand-in (fp32 radix-2, CPU) n_fft {n_fft}: worst r {worst:.3f}, bar {4 * worst:.3f}")
        # (the yardstick itself: per bin, with no filter to average over, the 9 to 11 stages of an fp32 radix-2 FFT leave up to a
        # unit of 2^-23 of the frame's energy each)
        assert 1.0 < worst < 16.0
        out[n_fft] = (per, 4.0 * worst)
    return out


@pytest.mark.parametrize("n_fft", sorted(RES))
def test_magnitudes_against_float64(ref, n_fft):
    per, bar = ref[n_fft]
    cases = CASES[n_fft]
    got, intact = R.run_magnitude([per[c][0] for c in cases], *RES[n_fft])          # 30 clips: one launch
    assert intact
    bad = []
    for c, S in zip(cases, got):
        _x, S64, norms = per[c]
        assert S.shape == S64.shape and not np.isnan(S).any(), c
        r = R.error_stat(S, S64, norms)
        print(f"stftd_error n_fft {n_fft:4d} {c[0]:10s} T {c[1]:5d} F {S64.shape[1]:3d}  r {r:.3f}  (bar {bar:.3f})")
        if not r <= bar:
            bad.append((c, r))
    assert not bad, bad


DIST_LENGTHS = (1025, 3001, 6007)
DIST_CASES = [(name, T) for name in R.BROADBAND for T in DIST_LENGTHS] + [("noise", 24000)]


@pytest.fixture(scope="module")
def dist_ref():
    """Per case: (estimate, target, float64 total, float64 components); and the bar."""
    out, worst = {}, 0.0
    for name, T in DIST_CASES:
        y = R.signal(name, T, seed=3)
        x = R.estimate_of(name, y)
        d64, c64 = R.distance64(x, y)
        d32, c32 = R.standin_distance_fp32(x, y)
        rel = max(abs(d32 - d64) / d64, float((np.abs(c32 - c64) / c64).max()))
        worst = max(worst, rel)
        out[(name, T)] = (x, y, d64, c64)
    bar = min(4.0 * worst, 1e-5)
    print(f"stftd distance stand-in (torch.stft fp32, CPU): worst relative error {worst:.3e}, bar {bar:.3e}")
    assert 1e-8 < worst < 1e-5
    return out, bar


def test_distance_values_against_float64_on_the_broadband_cases(dist_ref):
    cases, bar = dist_ref
    got, intact = R.run_distance([cases[c][0] for c in DIST_CASES], [cases[c][1] for c in DIST_CASES])
    assert intact
    bad = []
    for c, g in zip(DIST_CASES, got):
        _x, _y, d64, c64 = cases[c]
        assert np.isfinite(g).all(), c
        comps = g[1:].reshape(-1, 2).astype(np.float64)
        rel = max(abs(float(g[0]) - d64) / d64, float((np.abs(comps - c64) / c64).max()))
        print(f"stftd_distance {c[0]:10s} T {c[1]:5d}  d {float(g[0]):.7f}  float64 {d64:.7f}  worst relative error {rel:.3e}  (bar {bar:.3e})")
        assert g[0] == R.total_fp32(g[1:].reshape(-1, 2)), c           # the components add up to the total as defined
        if not rel <= bar:
            bad.append((c, rel))
    assert not bad, bad


def test_distance_is_made_of_the_magnitude_calls_bits():
    """The partial sums come from the magnitudes the spectrogram mode writes: sc and mag recomputed in float64 from the two magnitude
    calls agree with the distance call to fp32 summation error (n 2^-24 at the worst)."""
    T = 3001
    y = R.signal("noise", T, seed=5)
    x = R.estimate_of("noise", y)
    (g,), ok = R.run_distance([x], [y])
    assert ok
    for r, (n_fft, hop, win) in enumerate(R.RESOLUTIONS):
        (X, Y), ok = R.run_magnitude([x, y], n_fft, hop, win)
        assert ok
        X, Y = X.astype(np.float64), Y.astype(np.float64)
        sc = np.sqrt(((Y - X) ** 2).sum()) / np.sqrt((Y ** 2).sum())
        mg = np.abs(np.log(Y) - np.log(X)).mean()
        assert abs(float(g[1 + 2 * r]) - sc) <= 2e-6 * sc and abs(float(g[2 + 2 * r]) - mg) <= 2e-6 * mg, (r, g, sc, mg)


def test_a_sample_moves_only_the_frames_that_hold_it():
    n_fft, hop, win = RES[2048]
    T = 3001
    x = R.signal("noise", T, seed=4)
    sup = np.pad(np.arange(T), n_fft // 2, mode="reflect")[R.frame_index(T, n_fft, hop)]
    sup = np.where(R.window64(n_fft, win)[None, :] != 0, sup, -1)
    variants, touched = [x], []
    for n in (3, 700, 1500, 3000):
        y = x.copy()
        y[n] = y[n] + 0.25
        variants.append(y)
        touched.append((sup == n).any(axis=1))
    S, ok = R.run_magnitude(variants, n_fft, hop, win)
    assert ok
    for y, t in zip(S[1:], touched):
        assert 1 <= int(t.sum()) <= 6
        assert np.array_equal(y[:, ~t], S[0][:, ~t])                  # bit for bit
        assert bool((y[:, t] != S[0][:, t]).any(axis=0).all())        # and every frame that holds it moves


def test_exact_zeros_and_a_silent_pair_next_to_a_full_scale_one():
    T = 3001
    z = R.signal("silence", T)
    loud = (9.0 * R.signal("noise", T, seed=6)).astype(np.float32)
    louder = R.estimate_of("noise", loud)
    (alone,), ok = R.run_distance([z], [z])
    assert ok and bool((alone == 0.0).all()) and alone.shape == (7,)
    got, ok = R.run_distance([louder, z, louder], [loud, z, loud])
    assert ok and bool((got[1] == 0.0).all()) and np.array_equal(got[0], got[2]) and got[0][0] > 0
    for n_fft, hop, win in R.RESOLUTIONS:
        (S, Sl), ok = R.run_magnitude([z, loud], n_fft, hop, win)
        floor = np.sqrt(np.float32(1e-7))
        assert ok and bool((S == floor).all()) and bool((Sl >= floor).all())


def test_bit_identity_alone_in_a_batch_on_both_routes_and_over_the_workspace():
    """A pair alone; at positions 0, 31 and 64 of a call of 65 pairs of mixed lengths (descriptors through the workspace); in a call of
    three (descriptors in the argument block), whatever the workspace held before."""
    T = 3001
    y = R.signal("noise_tone", T, seed=8)
    x = R.estimate_of("noise_tone", y)
    (alone,), ok = R.run_distance([x], [y])
    assert ok and np.isfinite(alone).all()
    lengths = (1025, 1500, 2047, 4100)
    est, tgt = [], []
    for i in range(65):
        t = R.signal("noise", lengths[i % 4], seed=20 + i)
        tgt.append(t)
        est.append(R.estimate_of("noise", t))
    for pos in (0, 31, 64):
        est[pos], tgt[pos] = x, y
    for fill in (0xAB, 0xFF, 0x00):
        got, ok = R.run_distance(est, tgt, ws_fill=fill)
        assert ok and not any(np.isnan(g).any() for g in got)
        for pos in (0, 31, 64):
            assert np.array_equal(got[pos], alone), (fill, pos)
        three, ok = R.run_distance([est[1], x, est[2]], [tgt[1], y, tgt[2]], ws_fill=fill)
        assert ok and np.array_equal(three[1], alone) and np.array_equal(three[0], got[1]) and np.array_equal(three[2], got[2])
    # magnitudes: the same on both routes
    n_fft, hop, win = RES[512]
    (one,), ok = R.run_magnitude([x], n_fft, hop, win)
    many, ok2 = R.run_magnitude(est + [x] * 5, n_fft, hop, win)                       # 70 clips: through the workspace
    assert ok and ok2 and np.array_equal(many[-1], one) and np.array_equal(many[31], one)


def test_other_resolutions():
    """One resolution alone with win_length = n_fft, hop = n_fft and an odd win_length: check 1 once each."""
    x = R.signal("noise", 3001, seed=11)
    for n_fft, hop, win in ((512, 512, 512), (1024, 256, 599), (2048, 1, 2048)):
        xs = x[:1100] if hop == 1 else x
        (S,), ok = R.run_magnitude([xs], n_fft, hop, win)
        S64, norms = R.magnitude64(xs, n_fft, hop, win)
        worst = R.error_stat(R.standin_magnitude_fp32(xs, n_fft, hop, win), S64, norms)
        r = R.error_stat(S, S64, norms)
        print(f"stftd_error n_fft {n_fft:4d} hop {hop} win {win}  r {r:.3f}  (stand-in {worst:.3f})")
        assert ok and S.shape == S64.shape and r <= 4.0 * worst
