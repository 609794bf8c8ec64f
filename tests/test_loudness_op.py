"""The loudness kernels alone, through the C ABI (csrc/loudness.hip: wt_loudness, wt_normalize_rows_lufs), against the float64
definition of tests/loudness_ref.py.

Bound: per clip |L_gpu - L_ref64| may not exceed the error of a sequential fp32 lfilter evaluation of the same clip against
float64, or two fp32 ulps of the result where that is larger (tests/loudness_ref.py: bound); the relative threshold and every
momentary value are held to their own such bound, the gated block count is equal.  No block of any clip lies within 0.01 LU of
either gate in the reference (asserted), so no gate can flip inside the tolerance.

Lengths at 24 kHz, with C = wt_loudness_chunk(): the first block's edge (9599, 9600, 9601), the second's (11999, 12000), a chunk
more (9600 + C +- 1), the wave-scan edge (64 C - 1, 64 C, 64 C + 1: under 400 ms at 24 kHz, they read -inf; the same three at
8 kHz, where they hold 7 blocks and the edge shows in finite values), 3 * 64 C + 7, and about 10^6
samples (more than 64 waves of chunks: the cross-wave stage loads a second batch of totals); one clip of 1.5 s at each of six
other rates, a low-frequency-heavy clip (30 Hz + DC, where fp32 filtering is off by 10^-4 LU and more), a stereo clip.
Measured on an MI355X: profiles/loudness_error.txt."""
import math

import numpy as np
import pytest
import torch

from tests import loudness_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = R.SENTINEL
AMPLITUDES = (0.3, 0.02, 1.7)


def _chunk():
    from wavtokenizer_amd import _capi
    return int(_capi.lib.wt_loudness_chunk())


def _cases():
    """(name, rate, length, channels, kind)"""
    C = _chunk()
    lengths = [9599, 9600, 9601, 11999, 12000, 9600 + C - 1, 9600 + C + 1, 64 * C - 1, 64 * C, 64 * C + 1, 3 * 64 * C + 7, 1000003]
    cases = [("n%d" % n, 24000, n, 1, "noise") for n in lengths]
    cases += [("r%d" % fs, fs, fs * 3 // 2, 1, "noise") for fs in (8000, 11025, 16000, 22050, 44100, 48000)]
    cases += [("low", 24000, 72000, 1, "low"), ("stereo", 24000, 30001, 2, "noise")]
    cases += [("e%d" % n, 8000, n, 1, "noise") for n in (64 * C - 1, 64 * C, 64 * C + 1)]
    return cases


class Case:
    def __init__(self, j, name, fs, n, channels, kind):
        self.name, self.fs, self.n = name, fs, n
        if kind == "low":
            self.x = R.make_low_clip(n, fs, seed=7100 + j)
        elif channels == 2:
            self.x = np.stack([R.make_clip(n, seed=7100 + j, amplitude=0.3), R.make_clip(n, seed=7200 + j, amplitude=0.1)])
        else:
            self.x = R.make_clip(n, seed=7100 + j, amplitude=AMPLITUDES[j % 3])
        self.ref = R.loudness(self.x, fs)                                  # float64: L, threshold, count, l_j
        self.f32 = R.loudness(self.x, fs, np.float32)                      # the evaluation the bound comes from
        self.bound_L = R.bound(self.ref[0], self.f32[0])
        self.bound_G = R.bound(self.ref[1], self.f32[1])


@pytest.fixture(scope="module")
def cases():
    """Every clip on the CPU with its float64 and fp32 references, computed once and left unchanged."""
    assert 1 <= _chunk() <= 800
    return [Case(j, *c) for j, c in enumerate(_cases())]


@pytest.fixture(scope="module")
def measured(cases):
    """Per rate one wt_loudness over that rate's clips twice: in allocations of their own (16-byte aligned) and one float behind
    such a boundary.  Returns per case ((3,), l_j) aligned and shifted."""
    got = [None] * len(cases)
    for fs in sorted({c.fs for c in cases}):
        idx = [j for j, c in enumerate(cases) if c.fs == fs]
        on_gpu, shifted = [], []
        for j in idx:
            x = torch.from_numpy(cases[j].x)
            on_gpu.append(x.cuda())
            flat = x.reshape(-1)
            buf = torch.full((flat.shape[0] + 8,), float("nan"), dtype=torch.float32, device="cuda")
            buf[1:1 + flat.shape[0]] = flat.cuda()
            shifted.append(buf[1:1 + flat.shape[0]].view(x.shape))
        assert all(t.data_ptr() % 16 == 0 for t in on_gpu) and all(t.data_ptr() % 16 == 4 for t in shifted)
        out, blocks = R.measure(on_gpu + shifted, fs)
        for r, j in enumerate(idx):
            got[j] = ((out[r], blocks[r]), (out[len(idx) + r], blocks[len(idx) + r]))
    return got


def test_no_block_of_any_clip_lies_near_a_gate(cases):
    assert all(c.ref[2] > 0 for c in cases if c.name.startswith("e"))      # the wave-scan edge at 8 kHz is checked on finite values
    for c in cases:
        assert R.gate_margin(c.x, c.fs) >= 0.01, c.name
        assert c.ref[2] == c.f32[2], c.name                                # (the fp32 evaluation gates alike)


def test_loudness_threshold_count_and_momentary_within_the_bound(cases, measured):
    worst, worst_abs = 0.0, 0.0
    for c, ((out, blocks), (out_s, blocks_s)) in zip(cases, measured):
        L, G, count, l = c.ref
        err_L = abs(float(out[0]) - L) if math.isfinite(L) else 0.0
        err_G = abs(float(out[1]) - G) if math.isfinite(G) else 0.0
        bounds_l = [R.bound(a, b) for a, b in zip(l, c.f32[3])]
        err_l = [abs(float(g) - w) if math.isfinite(w) else 0.0 for g, w in zip(blocks, l)]
        print(f"loudness_error {c.name:9s} fs {c.fs:6d} n {c.n:8d}  L {float(out[0]):12.6f}  err {err_L:.3e}  bound {c.bound_L:.3e}  "
              f"fp32 lfilter err {abs(c.f32[0] - L) if math.isfinite(L) else 0.0:.3e}  threshold err {err_G:.3e}  blocks {int(out[2])}/{len(l)}  "
              f"momentary worst err {max(err_l, default=0.0):.3e}")
        if not math.isfinite(L):
            assert out[0] == -np.inf and out[1] == -np.inf and out[2] == 0, c.name
        else:
            assert err_L <= c.bound_L, (c.name, err_L, c.bound_L)
            assert err_G <= c.bound_G, (c.name, err_G, c.bound_G)
            assert float(out[2]) == count, (c.name, out[2], count)
            worst = max(worst, err_L / c.bound_L)
            worst_abs = max(worst_abs, err_L)
        assert blocks.shape == l.shape, c.name
        for j, (g, w, e, b) in enumerate(zip(blocks, l, err_l, bounds_l)):
            assert (g == w) if not math.isfinite(w) else (e <= b), (c.name, j, float(g), w, b)
        assert out_s.tobytes() == out.tobytes() and blocks_s.tobytes() == blocks.tobytes(), c.name     # the same bits off the 16-byte boundary
    print(f"loudness_error worst |L - L64| {worst_abs:.3e} LU, worst err / bound {worst:.3f}")


def test_gating_cases():
    fs = 24000
    rng = np.random.default_rng(41)
    steps = np.concatenate([0.1 * rng.standard_normal(fs), 0.001 * rng.standard_normal(2 * fs), np.zeros(fs)]).astype(np.float32)
    first = steps[:fs].copy()
    zeros = np.zeros(3 * fs, np.float32)
    tiny = np.full(3 * fs, 1e-5, np.float32)
    short = R.make_clip(9599, seed=43)
    clips = [steps, first, zeros, tiny, short]
    refs = [R.loudness(x, fs) for x in clips]
    f32 = [R.loudness(x, fs, np.float32) for x in clips]
    # the relative gate drops the quiet two seconds and the absolute gate the silence; the blocks that straddle the step stay
    # (white noise of 0.1 reads about -17.0; with these draws the issue's -17.727 / 10 blocks and -17.013 for the first second alone)
    assert abs(refs[0][0] + 17.727) < 0.15 and refs[0][2] == 10 and abs(refs[1][0] + 17.013) < 0.15 and refs[1][2] == 7
    assert refs[0][0] < refs[1][0] - 0.5
    assert R.gate_margin(steps, fs) >= 0.01 and R.gate_margin(first, fs) >= 0.01
    assert all(r[:3] == (-math.inf, -math.inf, 0) for r in refs[2:])
    assert refs[3][3].shape == (27,) and (refs[3][3] < -70.0 - 0.01).all()               # a constant: all of it under the high pass
    out, blocks = R.measure([torch.from_numpy(x).cuda() for x in clips], fs)
    for j in (0, 1):
        assert abs(float(out[j][0]) - refs[j][0]) <= R.bound(refs[j][0], f32[j][0]), j
        assert abs(float(out[j][1]) - refs[j][1]) <= R.bound(refs[j][1], f32[j][1]), j
        assert out[j][2] == refs[j][2], j
    for j in (2, 3, 4):
        assert out[j][0] == -np.inf and out[j][1] == -np.inf and out[j][2] == 0, j
    assert blocks[2].shape == (27,) and bool((blocks[2] == -np.inf).all()) and blocks[4].shape == (0,)
    assert bool((blocks[3] < -70.0).all())


def test_a_clip_has_the_same_bits_in_any_batch(cases):
    C = _chunk()
    c = next(c for c in cases if c.n == 3 * 64 * C + 7)
    fs, n = c.fs, c.n
    g = torch.from_numpy(c.x).cuda()
    alone, alone_blocks = R.measure([g], fs)
    short = [torch.from_numpy(R.make_clip(9000 + 97 * j, seed=900 + j)).cuda() for j in range(63)]
    many, many_blocks = R.measure([g] + short + [g.clone()], fs)              # 65 clips: the descriptors go through the workspace
    long = [torch.from_numpy(R.make_clip(100 * n, seed=990 + j)).cuda() for j in range(2)]
    among, among_blocks = R.measure([long[0], g, long[1]], fs)
    for what, got, blk in (("first of 65", many[0], many_blocks[0]), ("last of 65", many[64], many_blocks[64]),
                           ("among clips 100 x longer", among[1], among_blocks[1])):
        assert got.tobytes() == alone[0].tobytes(), what
        assert blk.tobytes() == alone_blocks[0].tobytes(), what
    assert math.isfinite(float(alone[0][0])) and abs(float(alone[0][0]) - c.ref[0]) <= c.bound_L
    for k in (0, 2):                                                             # (and the long ones are right themselves)
        x = long[k // 2].cpu().numpy()
        want, want32 = R.loudness(x, fs), R.loudness(x, fs, np.float32)
        assert abs(float(among[k][0]) - want[0]) <= R.bound(want[0], want32[0]) and among[k][2] == want[2], k
    # the normalised row and its scale
    row = g.clone()[None]
    s_alone = R.normalize_rows_lufs(row, [n], fs, -23.0)
    rows65 = torch.full((65, n + 5), SENTINEL, dtype=torch.float32, device="cuda")
    lens = [n] + [int(s.shape[0]) for s in short] + [n]
    for j, clip in enumerate([g] + short + [g]):
        rows65[j, :clip.shape[0]] = clip
    s65 = R.normalize_rows_lufs(rows65, lens, fs, -23.0)
    rows3 = torch.full((3, 100 * n), SENTINEL, dtype=torch.float32, device="cuda")
    rows3[0], rows3[1, :n], rows3[2] = long[0], g, long[1]
    s3 = R.normalize_rows_lufs(rows3, [100 * n, n, 100 * n], fs, -23.0)
    for what, got, sc in (("first of 65", rows65[0, :n], s65[0]), ("last of 65", rows65[64, :n], s65[64]),
                          ("among rows 100 x longer", rows3[1, :n], s3[1])):
        assert torch.equal(got, row[0]), what
        assert sc.cpu().numpy().tobytes() == s_alone[0].cpu().numpy().tobytes(), what
    assert bool((rows65[0, n:] == SENTINEL).all()) and bool((rows3[1, n:] == SENTINEL).all())
    assert not torch.equal(row[0], g)


@pytest.mark.parametrize("target", [-23.0, -16.0])
def test_normalize_rows_lufs(cases, target):
    fs = 24000
    C = _chunk()
    pick = [c for c in cases if c.fs == fs and c.x.ndim == 1 and c.n in (9600, 12000, 9600 + C + 1, 3 * 64 * C + 7, 72000)]
    assert len(pick) == 5
    xs = [c.x for c in pick] + [R.make_clip(5000, seed=61), np.zeros(20000, np.float32)]       # a short row and a silent row
    lens = [x.shape[0] for x in xs]
    rows = torch.full((len(xs), max(lens) + 3), SENTINEL, dtype=torch.float32, device="cuda")
    for r, x in enumerate(xs):
        rows[r, :lens[r]] = torch.from_numpy(x).cuda()
    scales = R.normalize_rows_lufs(rows, lens, fs, target).cpu().numpy()
    rows = rows.cpu().numpy()
    for r, x in enumerate(xs):
        d = scales[r]
        assert d.dtype == np.float32
        if r < len(pick):
            want = 10.0 ** ((pick[r].ref[0] - target) / 20.0)
            tol = (math.log(10.0) / 20.0) * pick[r].bound_L + 2.0 ** -23
            assert abs(float(d) - want) <= tol * want, (lens[r], float(d), want)
            assert d != 1.0
        else:
            assert d == 1.0, lens[r]                                            # no loudness: the row is left as it is
        assert rows[r, :lens[r]].tobytes() == (x / d).astype(np.float32).tobytes(), lens[r]      # one IEEE division per sample
        assert bool((rows[r, lens[r]:] == SENTINEL).all()), lens[r]            # columns past n_b keep the sentinel


def test_the_normalised_row_reads_the_target(cases):
    """Measured again, a normalised row reads the target within its bound, the rounding of d (2^-24 relative: 20 log10(1 + 2^-24)
    LU), that of the divisions (at most as much again) and the two ulps of the second reading."""
    fs, target = 24000, -23.0
    c = next(c for c in cases if c.name == "low")
    row = torch.from_numpy(c.x).cuda()[None].clone()
    R.normalize_rows_lufs(row, [c.n], fs, target)
    out, _blocks = R.measure([row[0]], fs, momentary=False)
    tol = c.bound_L + 2 * 20.0 * math.log10(1.0 + 2.0 ** -24) + 2 * R.ulp32(target)
    assert abs(float(out[0][0]) - target) <= tol, (float(out[0][0]), tol)
