"""The ragged overlap-add kernel (csrc/audio.hip overlap_add_ragged_kernel, wt_overlap_add_ragged) alone, through ctypes, without a
model: one launch over recordings of different frame lengths, strides and lengths whose frames lie scattered through a NaN-filled
arena as decode calls would leave them (a pitch above the frame length, something else behind each frame's samples), against the
oracle pinned to the reference's _linear_overlap_add (bit for bit), against the stored outputs of the reference itself, against a
float64 evaluation with a derived bound, and for what it must leave unread and unwritten.

The descriptor's weight table is what the reference builds: the triangle over the length of its FIRST frame, min(frame_len, total)
entries (a recording shorter than a segment has one frame, and the reference's triangle is that frame's)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import audio_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (frame_len, stride, total)
CASES = [(8, 8, 8), (8, 8, 24), (8, 6, 20), (8, 3, 17),
         (8, 1, 12),                 # eight deep, seven short trailing frames
         (257, 100, 1000),           # crosses the 256-output block edges
         (1200, 900, 2500), (1200, 1199, 3000),
         (4800, 3600, 3601)]         # the last frame is one sample
CANARY = -12345.5


def triangle(n):
    """The reference's weights (encoder/utils.py:46-47), from the same torch.linspace, as audio.linear_overlap_add builds them."""
    t = torch.linspace(0, 1, n + 2, dtype=torch.float32)[1:-1]
    return 0.5 - (t - 0.5).abs()


def make_frames(case, seed):
    flen, stride, total = case
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(min(flen, total - off)).astype(np.float32) for off in range(0, total, stride)]


class Launch:
    """One wt_overlap_add_ragged launch over recordings = [(case, frames, weight table (numpy))]: the frames go into a NaN-filled
    arena in a shuffled order at pitches above their length, the outputs into one buffer with canaries around each."""

    def __init__(self, recordings, seed=0):
        from wavtokenizer_amd import _capi
        rng = np.random.default_rng(seed)
        slots = [(r, f) for r, (_c, frames, _w) in enumerate(recordings) for f in range(len(frames))]
        order = rng.permutation(len(slots))
        pos, where = 3, {}
        for n, k in enumerate(order):
            r, f = slots[k]
            where[(r, f)] = pos
            pos += recordings[r][0][0] + 5 + n % 7           # a pitch above frame_len: NaN lies behind every frame, short or full
        arena = np.full(pos + 8, np.nan, np.float32)
        for (r, f), p in where.items():
            x = recordings[r][1][f]
            arena[p:p + len(x)] = x
        self.arena = torch.from_numpy(arena).cuda()
        ptrs, first = [], []
        for r, (_c, frames, _w) in enumerate(recordings):
            first.append(len(ptrs))
            ptrs += [self.arena.data_ptr() + 4 * where[(r, f)] for f in range(len(frames))]
        self.table = torch.tensor(ptrs, dtype=torch.int64).cuda()
        self.weights = [torch.from_numpy(w).cuda() for _c, _f, w in recordings]
        self.out_off, pos = [], 7
        for (flen, stride, total), _f, _w in recordings:
            self.out_off.append(pos)
            pos += total + 5
        self.out = torch.full((pos + 9,), CANARY, dtype=torch.float32, device="cuda")
        B = len(recordings)
        descs = (_capi.WtOverlapAddClip * B)()
        for d, ((flen, stride, total), frames, _w), fi, w, oo in zip(descs, recordings, first, self.weights, self.out_off):
            d.rows, d.n_frames, d.frame_len, d.stride, d.total = self.table.data_ptr() + 8 * fi, len(frames), flen, stride, total
            d.weight, d.out = w.data_ptr(), self.out.data_ptr() + 4 * oo
        nbytes = int(_capi.lib.wt_overlap_add_ragged_workspace_bytes(B))
        ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        _capi.check(_capi.lib.wt_overlap_add_ragged(descs, B, ctypes.c_void_p(ws.data_ptr()),
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "wt_overlap_add_ragged")
        torch.cuda.synchronize()
        self.totals = [c[2] for c, _f, _w in recordings]
        self.workspace, self.behind_workspace = ws[:nbytes], ws[nbytes:]

    def result(self, r):
        return self.out[self.out_off[r]:self.out_off[r] + self.totals[r]].cpu().numpy()

    def canaries_intact(self):
        mask = torch.ones(self.out.numel(), dtype=torch.bool, device="cuda")
        for o, n in zip(self.out_off, self.totals):
            mask[o:o + n] = False
        return bool((self.out[mask] == CANARY).all())


def _recordings(cases=CASES, seed=50):
    return [(c, make_frames(c, seed + j), triangle(min(c[0], c[2])).numpy()) for j, c in enumerate(cases)]


@pytest.fixture(scope="module")
def table():
    recs = _recordings()
    return recs, Launch(recs)


def test_one_launch_is_the_reference_loop_of_each_recording(table):
    recs, run = table
    assert [len(f) for _c, f, _w in recs] == [1, 3, 4, 6, 12, 10, 3, 3, 2]
    assert [len(f[-1]) for _c, f, _w in recs] == [8, 8, 2, 2, 1, 100, 700, 602, 1]
    assert [sum(len(x) < c[0] for x in f) for c, f, _w in recs][4] == 7                     # seven short trailing frames
    for r, (case, frames, _w) in enumerate(recs):
        want = audio_ref.linear_overlap_add(frames, case[1])                                 # (i) pinned to the reference
        got = run.result(r)
        assert want.shape == got.shape == (case[2],) and want.dtype == got.dtype
        assert np.array_equal(got, want), (case, int((got != want).sum()))
    # (v) nothing outside out[0, total) was written, nothing behind a frame's samples was read
    assert run.canaries_intact()
    assert not any(np.isnan(run.result(r)).any() for r in range(len(recs)))
    assert bool((run.workspace == 0xAB).all())              # (up to 64 recordings travel with the launch)


def test_the_library_helper_gives_the_same_bits(table):
    from wavtokenizer_amd import audio
    recs, run = table
    for r, (case, frames, _w) in enumerate(recs):
        got = audio.linear_overlap_add([torch.from_numpy(f).cuda() for f in frames], case[1]).cpu().numpy()
        assert np.array_equal(run.result(r), got), case


def test_against_float64(table):
    recs, run = table
    for r, ((flen, stride, total), frames, w) in enumerate(recs):
        num, den, mag, cover = (np.zeros(total) for _ in range(4))
        w64 = w.astype(np.float64)
        for f, x in enumerate(frames):
            o = f * stride
            num[o:o + len(x)] += w64[:len(x)] * x
            mag[o:o + len(x)] += np.abs(w64[:len(x)] * x)
            den[o:o + len(x)] += w64[:len(x)]
            cover[o:o + len(x)] += 1
        assert cover.min() >= 1 and cover.max() == -(-min(flen, total) // stride)
        # n rounded products, n - 1 sums twice (numerator and weight sum), one division, to first order
        bound = (2 * cover + 2) * 2.0 ** -24 * mag / den
        err = np.abs(run.result(r).astype(np.float64) - num / den)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"overlap_add_ragged {(flen, stride, total)}: depth {int(cover.max())}, max err / bound {worst:.3f}")
        assert bool((err <= bound).all()), ((flen, stride, total), worst)


def test_each_recording_alone_and_in_every_slot(table):
    recs, run = table
    n = len(recs)
    for r in range(n):
        alone = Launch([recs[r]], seed=100 + r)                                              # (iv) B = 1
        assert np.array_equal(alone.result(0), run.result(r)), recs[r][0]
        assert alone.canaries_intact()
    for shift in range(1, n):
        order = [(j + shift) % n for j in range(n)]
        turned = Launch([recs[j] for j in order], seed=200 + shift)
        for slot, j in enumerate(order):
            assert np.array_equal(turned.result(slot), run.result(j)), (shift, recs[j][0])
        assert turned.canaries_intact()


def test_the_stored_reference_outputs():
    """(ii) tests/golden/overlap_add.npz holds outputs of the reference function itself.  A ragged descriptor is a recording cut
    by segment_plan, n_frames = ceil(total / stride); three stored cases have frames that reach further (cases 0, 1 and 4: a last
    frame longer than the stride), and run on the longest prefix of their output that is such a recording, stride * n_frames
    samples, with the case's own triangle.  Every batch row of a case is a recording of the launch."""
    z = np.load(os.path.join(HERE, "golden", "overlap_add.npz"))
    recs, wants, full = [], [], 0
    ci = 0
    while f"case{ci}_meta" in z:
        nf, fl, ll, st, B = (int(v) for v in z[f"case{ci}_meta"])
        frames = [z[f"case{ci}_frame{i}"] for i in range(nf)]
        want = z[f"case{ci}_out"]
        total = min(st * (nf - 1) + ll, st * nf)
        full += total == want.shape[-1]
        for b in range(B):
            cut = [f[b, 0][:max(0, min(f.shape[-1], total - i * st))] for i, f in enumerate(frames)]
            assert all(len(c) for c in cut)
            recs.append(((fl, st, total), cut, triangle(fl).numpy()))
            wants.append(want[b, 0, :total])
        ci += 1
    assert ci == 7 and full == 4 and len(recs) == 14
    run = Launch(recs, seed=7)
    for r, want in enumerate(wants):
        assert np.array_equal(run.result(r), want), (r, recs[r][0])
    assert run.canaries_intact()


def test_more_recordings_than_travel_as_kernel_arguments():
    """Up to 64 descriptors go with the launch, more are uploaded through the workspace: 70 recordings in one launch equal the same
    recordings in launches of 35."""
    small = [c for c in CASES if c[2] <= 1000]
    recs = _recordings([small[j % len(small)] for j in range(70)], seed=300)
    big = Launch(recs, seed=1)
    assert not bool((big.workspace == 0xAB).all())          # (the descriptors were uploaded)
    for part in (range(0, 35), range(35, 70)):
        half = Launch([recs[j] for j in part], seed=2)
        for slot, j in enumerate(part):
            assert np.array_equal(half.result(slot), big.result(j)), j
    for j in (0, 5, 63, 64, 69):
        assert np.array_equal(big.result(j), audio_ref.linear_overlap_add(recs[j][1], recs[j][0][1])), j
    assert big.canaries_intact()
