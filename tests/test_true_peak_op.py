"""The true-peak kernel alone, through the C ABI (csrc/r128.hip: wt_true_peak), against the float64 definition of tests/r128_ref.py.

Bound: |got - want| <= (48 / F + 1) * 2^-24 * max_p sum_k |h[p + F k]| * max |x|, the standard bound of a 48 / F-term fp32 dot
product (every interpolated value is one; the maximum of values within a bound of their exact ones is within it of the exact
maximum).  The sample peak is exact and has the bits of wt_level's peak; the true peak is never below it.

Clips, with T = wt_true_peak_tile(): at 8000, 24000, 44100 (F = 4), 96000 (F = 2) and 192000 Hz (F = 1: the true peak is the
sample peak, bit for bit) the lengths 1, 5, 6, 7, 12, 13 (around the halo of 6 and of 12 samples), T - 1, T, T + 1, 2 T + 3, mono,
three of them also with two channels; one clip of 3 s; clips whose largest sample is the first, the last, on either side of a
tile edge, or in the second channel alone; fs / 4 sines of amplitude 0.5 (EBU Tech 3341, cases 15-18).  Every clip is measured
in an allocation of its own in one batch per rate, alone, in a batch of 3, in a batch of 70 (the descriptors then travel through
the workspace) and as a view one float off 16-byte alignment inside a buffer that holds 1e30 on both sides (a halo read past the
clip would show).  Observed errors on an MI355X: profiles/r128_error.txt."""
import math

import numpy as np
import pytest
import torch

from tests import loudness_ref as R
from tests import r128_ref as Q

pytestmark = pytest.mark.gpu

RATES = (8000, 24000, 44100, 96000, 192000)
PHASES = (0.0, 45.0, 60.0, 67.5)


def _tile():
    from wavtokenizer_amd import _capi
    return int(_capi.lib.wt_true_peak_tile())


class Case:
    def __init__(self, name, fs, x):
        self.name, self.fs, self.x = name, fs, np.ascontiguousarray(x, dtype=np.float32)
        self.tp, self.sp, self.bound = Q.true_peak(self.x, fs)             # float64 on the fp32 samples and taps


def _spiked(n, seed, where, channels=1, channel=0):
    x = np.stack([R.make_clip(n, seed=seed + c, amplitude=0.05) for c in range(channels)])
    x = np.clip(x, -0.4, 0.4)
    x[channel, where] = -0.9
    return x if channels > 1 else x[0]


def _cases():
    T = _tile()
    out, seed = [], 8100
    for fs in RATES:
        for n in (1, 5, 6, 7, 12, 13, T - 1, T, T + 1, 2 * T + 3):
            seed += 1
            out.append(Case("n%d" % n, fs, R.make_clip(n, seed=seed, amplitude=(0.3, 0.02, 1.7)[seed % 3])))
        for n in (7, T + 1, 2 * T + 3):
            seed += 1
            out.append(Case("s%d" % n, fs, np.stack([R.make_clip(n, seed=seed, amplitude=0.3), R.make_clip(n, seed=seed + 500, amplitude=0.2)])))
    out.append(Case("long", 24000, R.make_clip(72001, seed=8001, amplitude=0.3)))
    out.append(Case("longs", 44100, np.stack([R.make_clip(132300, seed=8002, amplitude=0.1), R.make_clip(132300, seed=8003, amplitude=0.3)])))
    for fs in (24000, 96000):
        n = 2 * T + 3
        out += [Case("first", fs, _spiked(n, 8010, 0)), Case("last", fs, _spiked(n, 8011, n - 1)), Case("edge-", fs, _spiked(n, 8012, T - 1)),
                Case("edge+", fs, _spiked(n, 8013, T)), Case("second", fs, _spiked(n, 8014, T + 5, channels=2, channel=1))]
    for fs in (8000, 24000, 44100):
        for ph in PHASES:
            # whole periods (a clip cut inside a period ends in a step, whose overshoot is a true peak of its own: -5.44 dBTP at 45 degrees)
            out.append(Case("sine%g" % ph, fs, 0.5 * np.sin(2 * np.pi * 0.25 * np.arange(4 * (fs // 16)) + math.radians(ph))))
    return out


@pytest.fixture(scope="module")
def cases():
    """Every clip on the CPU with its float64 reference, computed once and left unchanged."""
    assert _tile() > 24
    return _cases()


def _guarded(x: torch.Tensor) -> torch.Tensor:
    """x as a view at 4 bytes past a 16-byte boundary inside a buffer of 1e30, planes 5 floats apart."""
    C, n = (1, x.shape[0]) if x.dim() == 1 else x.shape
    pitch = n + 5
    buf = torch.full((33 + C * pitch + 32,), 1e30, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[33:33 + C * pitch].view(C, pitch)[:, :n]
    view.copy_(x.view(C, n))
    return view[0] if x.dim() == 1 else view


@pytest.fixture(scope="module")
def measured(cases):
    """Per case {"batch", "alone", "guard", "b3", "b70"}: (2,) fp32 each."""
    got = [dict() for _ in cases]
    for fs in RATES:
        idx = [j for j, c in enumerate(cases) if c.fs == fs]
        on_gpu = [torch.from_numpy(cases[j].x).cuda() for j in idx]
        assert all(t.data_ptr() % 16 == 0 for t in on_gpu)
        guard = [_guarded(t) for t in on_gpu]
        assert all(t.data_ptr() % 16 == 4 for t in guard)
        for key, out in (("batch", Q.measure_true_peak(on_gpu, fs)), ("guard", Q.measure_true_peak(guard, fs))):
            for r, j in enumerate(idx):
                got[j][key] = out[r]
        for r, j in enumerate(idx):
            got[j]["alone"] = Q.measure_true_peak([on_gpu[r]], fs)[0]
        for r0 in range(0, len(idx), 3):
            out = Q.measure_true_peak(on_gpu[r0:r0 + 3], fs)
            for r in range(out.shape[0]):
                got[idx[r0 + r]]["b3"] = out[r]
        order = [(3 * k) % len(idx) for k in range(70)] + list(range(len(idx)))       # 70 and more: through the workspace
        out = Q.measure_true_peak([on_gpu[r] for r in order], fs)
        for pos, r in enumerate(order):
            prev = got[idx[r]].setdefault("b70", out[pos])
            assert prev.tobytes() == out[pos].tobytes(), (cases[idx[r]].name, fs, "two places of one batch")
    return got


def test_true_peak_within_the_dot_product_bound(cases, measured):
    worst = 0.0
    for c, g in zip(cases, measured):
        tp, sp = float(g["batch"][0]), float(g["batch"][1])
        err = abs(tp - c.tp)
        print(f"true_peak_error {c.name:8s} fs {c.fs:6d} n {c.x.shape[-1]:7d} ch {c.x.ndim}  dBTP {Q.db(tp):9.4f}  sample {Q.db(sp):9.4f} dBFS  "
              f"err {err:.3e}  bound {c.bound:.3e}")
        assert err <= c.bound, (c.name, c.fs, err, c.bound)
        assert sp == c.sp, (c.name, c.fs)                                  # a maximum of fp32 values: exact
        assert tp >= sp, (c.name, c.fs)
        if c.bound > 0:
            worst = max(worst, err / c.bound)
    print(f"true_peak_error worst err / bound {worst:.3f}")


def test_sample_peak_has_the_bits_of_wt_level_and_f1_is_the_sample_peak(cases, measured):
    from wavtokenizer_amd import audio
    level = audio.level_many([torch.from_numpy(c.x).reshape(-1).cuda() for c in cases]).cpu().numpy()
    for c, g, lv in zip(cases, measured, level):
        assert g["batch"][1].tobytes() == lv[0].tobytes(), (c.name, c.fs)
        if c.fs == 192000:
            assert g["batch"][0].tobytes() == g["batch"][1].tobytes(), c.name


def test_quarter_rate_sines_read_inside_the_tolerance_of_tech_3341(cases, measured):
    seen = 0
    for c, g in zip(cases, measured):
        if c.name.startswith("sine"):
            seen += 1
            assert -6.4 <= Q.db(float(g["batch"][0])) <= -5.8, (c.name, c.fs, Q.db(float(g["batch"][0])))
    assert seen == 12


def test_peak_position_cases(cases, measured):
    seen = 0
    for c, g in zip(cases, measured):
        if c.name in ("first", "last", "edge-", "edge+", "second"):
            seen += 1
            assert float(g["batch"][1]) == float(np.float32(0.9)), (c.name, c.fs)
            assert float(g["batch"][0]) >= float(np.float32(0.9)) and abs(float(g["batch"][0]) - c.tp) <= c.bound, (c.name, c.fs)
    assert seen == 10


def test_same_bits_alone_in_batches_through_the_workspace_route_and_misaligned_between_1e30(cases, measured):
    for c, g in zip(cases, measured):
        for key in ("alone", "guard", "b3", "b70"):
            assert g[key].tobytes() == g["batch"].tobytes(), (c.name, c.fs, key, g[key], g["batch"])
