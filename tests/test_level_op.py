"""The level kernels alone, through the C ABI (csrc/level.hip: wt_level, wt_normalize_rows, wt_scale_rows): the peak against
numpy (exact), the rms against float64 within the derived bound of tests/level_ref.py, (3 + ceil(log2 n)) * 2^-24 relative, the
normalised rows against torch's fp32 expression on the CPU (bit for bit), batch invariance, and what must stay untouched.

Lengths: the wave and block edges, one chunk - 1 / one chunk / one chunk + 1 / 3 chunks + 7, and 256 chunks / 256 chunks + 1: up to
256 chunk partials are folded by the finishing workgroup's butterfly alone, from 257 on a pairwise pass through the workspace runs
first; the last two are also the clips of about 10^6 samples.
Measured on an MI355X: profiles/level_error.txt."""
import ctypes

import numpy as np
import pytest
import torch

from tests import level_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def _chunk():
    from wavtokenizer_amd import _capi
    return int(_capi.lib.wt_level_chunk())


def _lengths():
    C = _chunk()
    return [1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 7, 256 * C, 256 * C + 1]


@pytest.fixture(scope="module")
def clips():
    """Per length the clip on the CPU (numpy fp32), computed once and left unchanged."""
    assert _chunk() == 4096
    return [R.make_clip(n, seed=500 + j, amplitude=(0.3, 0.02, 1.7)[j % 3]) for j, n in enumerate(_lengths())]


@pytest.fixture(scope="module")
def measured(clips):
    """One wt_level over every clip twice: in an allocation of its own (16-byte aligned: the wide loads) and one element behind
    such a boundary (the scalar loads)."""
    on_gpu = [torch.from_numpy(x).cuda() for x in clips]
    shifted = []
    for x in clips:
        buf = torch.full((x.shape[0] + 8,), float("nan"), dtype=torch.float32, device="cuda")
        buf[1:1 + x.shape[0]] = torch.from_numpy(x).cuda()
        shifted.append(buf[1:1 + x.shape[0]])
    assert all(t.data_ptr() % 16 == 0 for t in on_gpu) and all(t.data_ptr() % 16 == 4 for t in shifted)
    return R.level(on_gpu + shifted).cpu().numpy()


def test_peak_is_exact_and_rms_within_the_bound(clips, measured):
    worst = 0.0
    for j, x in enumerate(clips):
        n = x.shape[0]
        peak, rms = measured[j]
        assert peak == np.abs(x).max(), (n, peak)
        want = R.rms64(x)
        err = abs(float(rms) - want) / want
        t = torch.from_numpy(x)
        torch_err = abs(float(t.pow(2).mean().sqrt()) - want) / want
        print(f"level_error n {n:8d}  rms {rms:.9g}  err {err / R.U:6.3f} u  bound {R.rms_bound(n) / R.U:4.0f} u  "
              f"torch fp32 CPU err {torch_err / R.U:6.3f} u")
        assert err <= R.rms_bound(n), (n, err / R.U)
        worst = max(worst, err / R.rms_bound(n))
        assert measured[len(clips) + j].tobytes() == measured[j].tobytes(), n          # the same bits off the 16-byte boundary
    print(f"level_error worst err / bound {worst:.3f}")


def test_a_clip_has_the_same_bits_in_any_batch(clips):
    C = _chunk()
    x = clips[_lengths().index(3 * C + 7)]
    n = x.shape[0]
    g = torch.from_numpy(x).cuda()
    alone = R.level([g]).cpu().numpy()[0]
    short = [torch.from_numpy(R.make_clip(100 + 7 * j, seed=900 + j)).cuda() for j in range(63)]
    many = R.level([g] + short + [g.clone()]).cpu().numpy()                    # 65 clips: the descriptors go through the workspace
    long = [torch.from_numpy(R.make_clip(100 * n, seed=990 + j)).cuda() for j in range(2)]
    among = R.level([long[0], g, long[1]]).cpu().numpy()
    for what, got in (("first of 65", many[0]), ("last of 65", many[64]), ("among clips 100 x longer", among[1])):
        assert got.tobytes() == alone.tobytes(), what
    for k in (0, 1):                                                             # (and the long ones are right themselves)
        assert among[2 * k][0] == np.abs(long[k].cpu().numpy()).max()
        want = R.rms64(long[k].cpu().numpy())
        assert abs(float(among[2 * k][1]) - want) / want <= R.rms_bound(100 * n)
    # the normalised row and its scale, both modes
    for mode in (0, 1):
        row = g.clone()[None]
        s_alone = R.normalize_rows(row, [n], mode)
        rows65 = torch.full((65, n + 5), SENTINEL, dtype=torch.float32, device="cuda")
        lens = [n] + [int(s.shape[0]) for s in short] + [n]
        for j, c in enumerate([g] + short + [g]):
            rows65[j, :c.shape[0]] = c
        s65 = R.normalize_rows(rows65, lens, mode)
        rows3 = torch.full((3, 100 * n), SENTINEL, dtype=torch.float32, device="cuda")
        rows3[0], rows3[1, :n], rows3[2] = long[0], g, long[1]
        s3 = R.normalize_rows(rows3, [100 * n, n, 100 * n], mode)
        for what, got, sc in (("first of 65", rows65[0, :n], s65[0]), ("last of 65", rows65[64, :n], s65[64]),
                              ("among rows 100 x longer", rows3[1, :n], s3[1])):
            assert torch.equal(got, row[0]), (mode, what)
            assert sc.cpu().numpy().tobytes() == s_alone[0].cpu().numpy().tobytes(), (mode, what)
        assert bool((rows65[0, n:] == SENTINEL).all()) and bool((rows3[1, n:] == SENTINEL).all())
        assert float(s_alone[0]) == float(np.float32(alone[mode]) + np.float32(1e-8))     # the measurement is wt_level's


def _normalized(clips, idx, mode, gain=1.0):
    """wt_normalize_rows over clips[idx] as the rows of one sentinel-filled tensor: (rows on the CPU, scales on the CPU, lengths)."""
    lens = [clips[j].shape[0] for j in idx]
    rows = torch.full((len(idx), max(lens) + 3), SENTINEL, dtype=torch.float32, device="cuda")
    for r, j in enumerate(idx):
        rows[r, :lens[r]] = torch.from_numpy(clips[j]).cuda()
    scales = R.normalize_rows(rows, lens, mode, gain)
    return rows.cpu(), scales.cpu(), lens


def _groups():
    """Row groups of one call each: the lengths up to 3 chunks + 7 together, the two of about 10^6 samples together."""
    n = len(_lengths())
    return [list(range(n - 2)), [n - 2, n - 1]]


def test_peak_mode_with_gain_one_is_torchs_expression(clips):
    for idx in _groups():
        rows, scales, lens = _normalized(clips, idx, 0)
        for r, j in enumerate(idx):
            want, scale = R.peak_normalize(torch.from_numpy(clips[j]))
            assert torch.equal(rows[r, :lens[r]], want), (lens[r], int((rows[r, :lens[r]] != want).sum()))
            assert float(scales[r]) == float(scale), lens[r]
            assert bool((rows[r, lens[r]:] == SENTINEL).all()), lens[r]            # columns past n_b keep the sentinel


def test_peak_mode_with_a_target_and_rms_mode(clips, measured):
    gain = R.gain_of(-3.0)
    assert gain != 1.0 and abs(gain - 0.70794576) < 1e-7
    idx = _groups()[0]
    rows, scales, lens = _normalized(clips, idx, 0, gain)
    for r, j in enumerate(idx):
        want, scale = R.peak_normalize(torch.from_numpy(clips[j]), gain)
        assert torch.equal(rows[r, :lens[r]], want) and float(scales[r]) == float(scale), lens[r]
    for idx in _groups():
        rows, scales, lens = _normalized(clips, idx, 1)
        for r, j in enumerate(idx):
            x = torch.from_numpy(clips[j])
            scale = torch.tensor(1e-8, dtype=torch.float32) + torch.tensor(measured[j][1])      # 1e-8 + wt_level's rms, in fp32
            assert float(scales[r]) == float(scale), lens[r]
            assert torch.equal(rows[r, :lens[r]], x / scale), lens[r]
            _y, ref_scale = R.rms_normalize(x)                                       # torch's own mean: within the bound, not bitwise
            assert abs(float(scale) - float(ref_scale)) <= 2 * R.rms_bound(lens[r]) * float(ref_scale), lens[r]
            assert bool((rows[r, lens[r]:] == SENTINEL).all()), lens[r]


def test_silence_negative_zero_and_a_denormal():
    n = 300
    special = np.zeros(n, np.float32)
    special[3], special[10], special[200] = -0.0, 1e-40, 0.25
    special[5] = -0.125
    assert np.signbit(special[3]) and 0 < special[10] < np.finfo(np.float32).tiny
    for mode in (0, 1):
        rows = torch.full((2, n + 2), SENTINEL, dtype=torch.float32, device="cuda")
        rows[0, :n] = 0.0
        rows[1, :n] = torch.from_numpy(special).cuda()
        scales = R.normalize_rows(rows, [n, n], mode).cpu()
        rows = rows.cpu()
        assert bool((rows[0, :n] == 0).all()) and float(scales[0]) == float(np.float32(1e-8)), mode
        x = torch.from_numpy(special)
        if mode == 0:
            want, scale = R.peak_normalize(x)
            assert float(scales[1]) == float(scale)
        else:
            want = x / scales[1]
            assert abs(float(scales[1]) - (1e-8 + R.rms64(special))) <= R.rms_bound(n) * float(scales[1])
        assert rows[1, :n].numpy().tobytes() == want.numpy().tobytes(), mode          # (bytes: the sign of the zero counts)
        assert np.signbit(rows[1, 3].numpy()) and float(rows[1, 10]) > 0
        assert bool((rows[:, n:] == SENTINEL).all())
    level = R.level([torch.from_numpy(special).cuda(), torch.zeros(n, device="cuda")]).cpu().numpy()
    assert level[0][0] == 0.25 and level[1].tolist() == [0.0, 0.0]


def test_scale_rows_is_the_torch_product_and_stops_at_the_length():
    lens = [1, 3, 4, 5, 1023, 1024, 1025, 4101]
    buf = torch.full((sum(n + 9 for n in lens) + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    rows, pos = [], 4
    for j, n in enumerate(lens):
        pos += j % 4                                                                  # every 4-byte alignment within 16 bytes
        rows.append(buf[pos:pos + n])
        rows[-1].copy_(torch.from_numpy(R.make_clip(n, seed=700 + j)).cuda())
        pos += n + 5
    before = buf.clone()
    scales = torch.tensor([0.37, 1.0, 3.1e-4, 511.0, 0.99, 1.0e-8 + 0.123, 2.5, 0.0625], dtype=torch.float32).cuda()
    R.scale_rows(rows, lens, scales)
    touched = torch.zeros_like(buf, dtype=torch.bool)
    for j, (row, n) in enumerate(zip(rows, lens)):
        off = (row.data_ptr() - buf.data_ptr()) // 4
        assert torch.equal(row, before[off:off + n] * scales[j]), n
        touched[off:off + n] = True
    assert torch.equal(buf[~touched], before[~touched])


def test_invalid_descriptors_touch_nothing():
    from wavtokenizer_amd import _capi
    lib, INVALID = _capi.lib, _capi.WT_ERR_INVALID
    x = torch.full((64,), 0.5, dtype=torch.float32, device="cuda")
    out = torch.full((2, 2), SENTINEL, dtype=torch.float32, device="cuda")
    ws = torch.zeros(int(lib.wt_level_workspace_bytes(2, 128)) + 16, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(mutate, B=2, workspace=ws.data_ptr()):
        descs = (_capi.WtLevelClip * 2)()
        for j, d in enumerate(descs):
            d.x, d.n, d.out = x.data_ptr(), 64, out.data_ptr() + 8 * j
        mutate(descs)
        return lib.wt_level(descs, B, ctypes.c_void_p(workspace), stream)

    def setter(j, field, value):
        return lambda descs: setattr(descs[j], field, value)

    for what, rc in (("n = 0", call(setter(1, "n", 0))), ("n < 0", call(setter(0, "n", -5))), ("null x", call(setter(1, "x", None))),
                     ("misaligned x", call(setter(0, "x", x.data_ptr() + 2))), ("null out", call(setter(1, "out", None))),
                     ("misaligned out", call(setter(1, "out", out.data_ptr() + 1))), ("B = 0", call(lambda d: None, B=0)),
                     ("null workspace", call(lambda d: None, workspace=None)),
                     ("misaligned workspace", call(lambda d: None, workspace=ws.data_ptr() + 4))):
        assert rc == INVALID, what
        assert b"wt_level" in lib.wt_last_error(), what
    assert lib.wt_level(None, 2, ctypes.c_void_p(ws.data_ptr()), stream) == INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())

    rows = torch.full((2, 64), 0.5, dtype=torch.float32, device="cuda")
    scales = torch.full((2,), SENTINEL, dtype=torch.float32, device="cuda")
    ws2 = torch.zeros(int(lib.wt_normalize_rows_workspace_bytes(2, 64)), dtype=torch.uint8, device="cuda")

    def norm(n=(64, 64), mode=0, gain=1.0, rows_ptr=rows.data_ptr(), T_pad=64):
        return lib.wt_normalize_rows(ctypes.c_void_p(rows_ptr), 2, T_pad, (ctypes.c_int64 * 2)(*n), mode, gain,
                                     ctypes.c_void_p(scales.data_ptr()), ctypes.c_void_p(ws2.data_ptr()), stream)

    for what, rc in (("n > T_pad", norm(n=(64, 65))), ("n = 0", norm(n=(0, 64))), ("mode", norm(mode=2)), ("gain 0", norm(gain=0.0)),
                     ("gain nan", norm(gain=float("nan"))), ("rms with a gain", norm(mode=1, gain=0.5)), ("null rows", norm(rows_ptr=None)),
                     ("misaligned rows", norm(rows_ptr=rows.data_ptr() + 2)), ("T_pad = 0", norm(T_pad=0))):
        assert rc == INVALID, what
    torch.cuda.synchronize()
    assert bool((rows == 0.5).all()) and bool((scales == SENTINEL).all())
    one = (ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(scales.data_ptr()))
    assert lib.wt_scale_rows(None, one[1], one[2], 1, 64, stream) == INVALID
    assert lib.wt_scale_rows(one[0], one[1], one[2], 0, 64, stream) == INVALID
    assert lib.wt_scale_rows(one[0], one[1], one[2], 1, 0, stream) == INVALID
