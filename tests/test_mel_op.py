"""The mel kernels (csrc/mel.hip) alone, through ctypes: clips in a NaN-filled arena, outputs between canaries, against the float64
definition (tests/mel_ref.py) with a bar that comes from an fp32 radix-2 stand-in run on the CPU in this test (never from the
kernel), and for what a frame, a clip and a call must not depend on.

Error statistic (check 1): r = max |M - M64| / (2^-23 (||fb[:, m]||_1 ||w x_f||_2 + M64)); the bar is 4 x the largest r the stand-in
reaches over the same cases (a higher radix, the split pass of a half-length real FFT and a fast sqrt reorder the rounding steps of
a radix-2 transform but do not multiply them).  Measured on an MI355X: profiles/mel_error.txt."""
import numpy as np
import pytest

from tests import mel_ref as R

pytestmark = pytest.mark.gpu

CASES = [(name, T) for name in R.SIGNALS for T in R.LENGTHS]


@pytest.fixture(scope="module")
def ref():
    """Per case: the clip, M64, the frame norms; and the bar."""
    out, worst = {}, 0.0
    for name, T in CASES:
        x = R.signal(name, T)
        M64, norms = R.mel64(x)
        r = R.error_stat(R.standin_fp32(x), M64, norms)
        worst = max(worst, r)
        out[(name, T)] = (x, M64, norms)
    print(f"mel stand-in (fp32 radix-2, CPU): worst r {worst:.3f}, bar {4 * worst:.3f}")
    assert 0.5 < worst < 4.0                     # (the yardstick itself: an fp32 FFT is a few units of 2^-23 of the frame's energy)
    return out, 4.0 * worst


@pytest.fixture(scope="module")
def launched(ref):
    """All cases in one linear and one log launch (49 clips: the argument-block path)."""
    cases, _bar = ref
    clips = [cases[c][0] for c in CASES]
    lin, ok1 = R.run(clips, log=False)
    log, ok2 = R.run(clips, log=True)
    return dict(zip(CASES, lin)), dict(zip(CASES, log)), ok1 and ok2


def test_linear_mel_against_float64(ref, launched):
    cases, bar = ref
    lin, _log, intact = launched
    assert intact
    bad = []
    for c in CASES:
        _x, M64, norms = cases[c]
        assert lin[c].shape == M64.shape and not np.isnan(lin[c]).any(), c
        r = R.error_stat(lin[c], M64, norms)
        print(f"mel_error {c[0]:10s} T {c[1]:5d} F {M64.shape[1]:3d}  r {r:.3f}  (bar {bar:.3f})")
        if not r <= bar:
            bad.append((c, r))
    assert not bad, bad


def test_log_mel_against_float64_on_the_broadband_cases(ref, launched):
    cases, bar = ref
    _lin, log, _intact = launched
    for c in CASES:
        if c[0] not in R.BROADBAND:
            continue
        _x, M64, norms = cases[c]
        bound, skip = R.log_bound(bar, M64, norms)
        assert int(skip.sum()) == 0, (c, int(skip.sum()))
        err = np.abs(log[c].astype(np.float64) - R.safe_log(M64))
        worst = float((err / bound).max())
        print(f"mel_log_error {c[0]:10s} T {c[1]:5d}  max err / bound {worst:.3f}")
        assert bool((err <= bound).all()), (c, worst)


def _zero_frames(T, tail=200, hop=256):
    return np.nonzero((R.frame_support(T, hop) < T - tail).all(axis=1))[0]


def test_frames_of_zeros(launched):
    _lin, log, _intact = launched
    floor = np.log(np.float32(1e-7))                                  # fp32
    seen = 0
    for T in (3000, 8453):
        L = log[("burst", T)]
        z = _zero_frames(T)
        assert len(z) >= 5
        vals = np.unique(L[:, z])
        assert vals.shape == (1,) and abs(float(vals[0]) - float(floor)) <= float(np.spacing(np.abs(floor))), (T, vals, floor)
        seen = vals[0]
    T = 3000
    silent, noise, sine = R.signal("silence", T), R.signal("noise", T), R.signal("sine", T)
    (La, Lnoise, Lsine), ok = R.run([silent, noise, sine])
    assert ok and bool((La == seen).all())
    d, ok = R.run([silent, silent, silent], [silent, noise, sine])
    assert ok and d[0] == 0.0
    # the silent side keeps its bits whatever it is paired with: the distance has the bits that the kernels' own summation order
    # (mel_ref.distance_fp32) gives for the constant against the other's own spectrogram.  A transform that packed the pair into
    # one complex FFT would put the silent side 2.9 off next to this noise, and 3e-4 off next to a -60 dB partner
    faint = (1e-3 * noise).astype(np.float32)
    (Lfaint,), ok = R.run([faint])
    dq, ok_q = R.run([silent], [faint])
    assert ok and ok_q
    for got, Lo in ((d[1], Lnoise), (d[2], Lsine), (dq[0], Lfaint)):
        want = R.distance_fp32(np.full_like(Lo, seen), Lo)
        assert got == want, (got, want)


def test_a_sample_moves_only_the_frames_that_hold_it():
    T = 3000
    x = R.signal("noise", T, seed=4)
    sup = R.frame_support(T, 256)
    variants, touched = [x], []
    for n in (3, 700, 1500, 2999):                                    # (3 also enters frame 0 through the reflection)
        y = x.copy()
        y[n] = y[n] + 0.25
        variants.append(y)
        touched.append((sup == n).any(axis=1))
    L, ok = R.run(variants)
    assert ok
    for y, t in zip(L[1:], touched):
        assert 1 <= int(t.sum()) <= 6
        assert np.array_equal(y[:, ~t], L[0][:, ~t])                  # bit for bit
        assert bool((y[:, t] != L[0][:, t]).any(axis=0).all())        # and every frame that holds it moves


PAIRS = [("noise / noisy copy", 3000), ("quiet / quiet", 3000), ("loud / -60 dB", 3000), ("noise / noisy copy", 8453), ("quiet / quiet", 513)]


def _pair(kind, T):
    if kind == "noise / noisy copy":
        a = R.signal("noise", T, seed=1)
        return a, (a + 1e-3 * np.random.default_rng(T).standard_normal(T)).astype(np.float32)
    if kind == "quiet / quiet":
        return R.signal("quiet", T, seed=1), R.signal("quiet", T, seed=2)
    return R.signal("noise", T, seed=1), (1e-3 * R.signal("noise", T, seed=2)).astype(np.float32)


def test_distance_against_its_own_spectrogram_and_against_float64(ref):
    _cases, bar = ref
    a = [_pair(k, T)[0] for k, T in PAIRS]
    b = [_pair(k, T)[1] for k, T in PAIRS]
    d, ok = R.run(a, b)
    La, ok_a = R.run(a)
    Lb, ok_b = R.run(b)
    assert ok and ok_a and ok_b
    for i, (k, T) in enumerate(PAIRS):
        n = La[i].size
        own = float(np.abs(La[i].astype(np.float64) - Lb[i].astype(np.float64)).mean())
        assert abs(float(d[i]) - own) <= n * 2.0 ** -24 * own, (k, T, d[i], own)
        assert d[i] == R.distance_fp32(La[i], Lb[i]), (k, T)          # and the bits of the kernels' own summation order
        # float64 definition: per entry ||La - Lb| - |La64 - Lb64|| <= |La - La64| + |Lb - Lb64|, each within its log bound: the
        # mean of the two sides' bounds
        (Ma, na), (Mb, nb) = R.mel64(a[i]), R.mel64(b[i])
        ba, sa = R.log_bound(bar, Ma, na)
        bb, sb = R.log_bound(bar, Mb, nb)
        assert not sa.any() and not sb.any()
        d64 = float(np.abs(R.safe_log(Ma) - R.safe_log(Mb)).mean())
        tol = float((ba + bb).mean())
        print(f"mel_distance {k:18s} T {T:5d}  d {float(d[i]):.6f}  float64 {d64:.6f}  |diff| {abs(float(d[i]) - d64):.2e}  tol {tol:.2e}")
        assert abs(float(d[i]) - d64) <= tol, (k, T)
        assert abs(d64 - R.distance64(a[i], b[i])) < 1e-12


def _invariance(clips, others, **kw):
    """clips alone, in a batch of 7 in two orders, and as clips 3 and 68 of a batch of 70 (descriptors through the workspace)."""
    assert len(clips) == 2 and len(others) == 5
    alone = [R.run([c], **kw)[0][0] for c in clips]
    alone_d = [R.run([c], [o], **kw)[0][0] for c, o in zip(clips, others)]
    seven = [clips[0], *others[:3], clips[1], *others[3:]]
    seven_b = [c[::-1].copy() for c in seven]
    seven_b[0], seven_b[4] = others[0], others[1]
    for order in (list(range(7)), [6, 4, 2, 0, 5, 3, 1]):
        got, ok = R.run([seven[j] for j in order], **kw)
        assert ok
        assert np.array_equal(got[order.index(0)], alone[0]) and np.array_equal(got[order.index(4)], alone[1]), order
        gd, ok = R.run([seven[j] for j in order], [seven_b[j] for j in order], **kw)
        assert ok and gd[order.index(0)] == alone_d[0] and gd[order.index(4)] == alone_d[1], order
    filler = others[0][:600]
    many = [filler] * 70
    many[3], many[68] = clips
    partner = [filler] * 70
    partner[3], partner[68] = others[0], others[1]
    for fill in (0xAB, 0x00):
        got, ok = R.run(many, ws_fill=fill, **kw)
        assert ok and np.array_equal(got[3], alone[0]) and np.array_equal(got[68], alone[1])
        assert not any(np.isnan(g).any() for g in got)
        gd, ok = R.run(many, partner, ws_fill=fill, **kw)
        assert ok and gd[3] == alone_d[0] and gd[68] == alone_d[1] and not np.isnan(gd).any()
        assert gd[0] == 0.0
    pd, ok = R.run([clips[1], clips[0]], [others[1], others[0]], **kw)
    assert ok and pd[0] == alone_d[1] and pd[1] == alone_d[0]


def test_batch_invariance_and_workspace_contents():
    clips = [R.signal("noise", 3000, seed=7), R.signal("sine_noise", 8453, seed=7)]
    others = [R.signal("quiet", 3000, seed=8), R.signal("noise", 8453, seed=8), R.signal("square", 1025), R.signal("noise", 513, seed=9),
              R.signal("burst", 1023)]
    _invariance(clips, others)


def test_other_hop_mels_and_rate(ref):
    """hop_length 100, n_mels 64 at 16 kHz: the linear check and the batch invariance once, on T = 3000 noise."""
    _cases, bar = ref
    kw = dict(sample_rate=16000, hop=100, n_mels=64)
    x = R.signal("noise", 3000, seed=11)
    (M,), ok = R.run([x], log=False, **kw)
    M64, norms = R.mel64(x, 16000, 100, 64)
    assert ok and M.shape == M64.shape == (64, 31)
    r = R.error_stat(M, M64, norms, 16000, 64)
    print(f"mel_error noise      T  3000 F  31  r {r:.3f}  (bar {bar:.3f}; 16 kHz, hop 100, 64 mels)")
    assert r <= bar
    others = [R.signal("quiet", 3000, seed=12), R.signal("noise", 3000, seed=13), R.signal("square", 1025), R.signal("noise", 513, seed=9),
              R.signal("burst", 1023)]
    _invariance([x, R.signal("sine_noise", 3000, seed=11)], others, **kw)
