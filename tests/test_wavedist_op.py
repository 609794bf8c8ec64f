"""The time-domain kernels (csrc/wavedist.hip) alone, through ctypes: pairs in a NaN-filled arena, outputs between canaries,
against the float64 definition (tests/wavedist_ref.py).  The bar is 4 x the worst error in dB of the fp32 three-pass stand-in run
on the CPU in this test over the same cases (never from the kernel), and never above 0.01 dB.
Measured on an MI355X: profiles/stftd_error.txt."""
import numpy as np
import pytest

from tests import wavedist_ref as R

pytestmark = pytest.mark.gpu


def _cases():
    blk = R.block()
    cases = []
    for T in (1, 63, 64, 65, blk - 1, blk, blk + 1, 100001):
        for sdr in (10.0, 40.0, 70.0, 100.0):
            cases.append((f"T {T:6d} {sdr:5.1f} dB", R.pair(T, sdr), False))
        p, t = R.pair(T, 40.0, seed=1)
        cases.append((f"T {T:6d} estimate = target", (t.copy(), t), False))
        for zm in (False, True):
            cases.append((f"T {T:6d} dc 0.5 on 0.01, zero_mean {int(zm)}", R.pair(T, 40.0, seed=2, level=0.01, dc=0.5), zm))
    return cases


@pytest.fixture(scope="module")
def ref():
    cases = _cases()
    want, worst = [], 0.0
    for _name, (p, t), zm in cases:
        w = R.measures64(p, t, zm)
        s = R.standin_fp32(p, t, zm)
        worst = max(worst, abs(s[0] - w[0]), abs(s[1] - w[1]))
        want.append(w)
    bar = min(4.0 * worst, 0.01)
    print(f"wavedist stand-in (fp32 three-pass, CPU): worst error {worst:.3e} dB, bar {bar:.3e} dB")
    assert 1e-7 < worst < 2.5e-3
    return cases, want, bar


def test_si_sdr_and_snr_against_float64(ref):
    cases, want, bar = ref
    bad = []
    for zm in (False, True):
        sel = [i for i, c in enumerate(cases) if c[2] == zm]
        got, intact = R.run([cases[i][1][0] for i in sel], [cases[i][1][1] for i in sel], zero_mean=zm)
        assert intact
        for i, g in zip(sel, got):
            assert np.isfinite(g).all(), cases[i][0]
            err = max(abs(float(g[0]) - want[i][0]), abs(float(g[1]) - want[i][1]))
            print(f"wavedist_error {cases[i][0]:42s} si_sdr {float(g[0]):10.5f} (float64 {want[i][0]:10.5f})  snr {float(g[1]):10.5f} "
                  f"(float64 {want[i][1]:10.5f})  worst {err:.2e} dB  (bar {bar:.2e})")
            if not err <= bar:
                bad.append((cases[i][0], err))
    assert not bad, bad


def test_exact_zeros_and_a_silent_pair_next_to_a_full_scale_one():
    z = np.zeros(5000, np.float32)
    p, t = R.pair(5000, 10.0, seed=3, level=0.9)
    for zm in (False, True):
        (alone,), ok = R.run([z], [z], zero_mean=zm)
        assert ok and alone[0] == 0.0 and alone[1] == 0.0
        got, ok = R.run([p, z, p, z[:1]], [t, z, t, z[:1]], zero_mean=zm)
        assert ok and bool((got[1] == 0.0).all()) and bool((got[3] == 0.0).all()) and np.array_equal(got[0], got[2])
        assert abs(float(got[0][0]) - 10.0) < 0.1


def test_bit_identity_alone_in_a_batch_on_both_routes_and_over_the_workspace():
    blk = R.block()
    p, t = R.pair(3 * blk + 17, 40.0, seed=4)
    lengths = (1, 65, blk, blk + 1, 5000)
    est, tgt = [], []
    for i in range(65):
        a, b = R.pair(lengths[i % 5], 20.0, seed=30 + i)
        est.append(a)
        tgt.append(b)
    for pos in (0, 31, 64):
        est[pos], tgt[pos] = p, t
    for zm in (False, True):
        (alone,), ok = R.run([p], [t], zero_mean=zm)
        assert ok and np.isfinite(alone).all()
        for fill in (0xAB, 0xFF, 0x00):
            got, ok = R.run(est, tgt, zero_mean=zm, ws_fill=fill)
            assert ok and not any(np.isnan(g).any() for g in got)
            for pos in (0, 31, 64):
                assert np.array_equal(got[pos], alone), (zm, fill, pos)
            three, ok = R.run([est[1], p, est[3]], [tgt[1], t, tgt[3]], zero_mean=zm, ws_fill=fill)
            assert ok and np.array_equal(three[1], alone) and np.array_equal(three[0], got[1]) and np.array_equal(three[2], got[3])


def test_scale_behaviour(ref):
    """A power-of-two gain on both signals moves no bit of SI-SDR while eps = 2^-23 stays below half an ulp of every sum: tested
    for gains 2^4 .. 2^40 on a 10 dB pair of 3000 samples at level 0.1 (its smallest sum, the residual energy, is about 1.9 at gain
    1, so 490 and more here, where half an ulp is 1.5e-5).  A gain g on the estimate alone leaves SI-SDR within the bar and moves SNR
    to what the definition gives for (g p, t)."""
    _cases_, _want, bar = ref
    p, t = R.pair(3000, 10.0, seed=5)
    gains = [2.0 ** k for k in (4, 5, 11, 24, 40)]
    got, ok = R.run([(g * p).astype(np.float32) for g in gains], [(g * t).astype(np.float32) for g in gains])
    assert ok
    for g, v in zip(gains[1:], got[1:]):
        assert v[0] == got[0][0] and v[1] == got[0][1], (g, v, got[0])
    gains = [1.0, 0.5, 3.0, 0.1]
    scaled = [(g * p).astype(np.float32) for g in gains]
    got, ok = R.run(scaled, [t] * len(gains))
    assert ok
    for g, q, v in zip(gains, scaled, got):
        want = R.measures64(q, t)
        assert abs(float(v[0]) - float(got[0][0])) <= bar and abs(float(v[0]) - want[0]) <= bar, (g, v, want)
        assert abs(float(v[1]) - want[1]) <= bar, (g, v, want)
    assert abs(float(got[1][1]) - float(got[0][1])) > 1.0                       # (SNR is not scale-invariant)
