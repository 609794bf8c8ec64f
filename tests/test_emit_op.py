"""The ragged emit kernel (csrc/audio.hip emit_kernel, wt_emit) alone: one launch over synthetic rows laid out as the decode
plans leave them ([B][pitch], something else behind each clip's samples) to nine rates, both channel counts, three layouts and both
sample types, against audio.convert_audio / audio.to_pcm16 of each clip alone (bit for bit), against a float64 evaluation of the
polyphase sum (derived bound, tests/emit_ref.py), and for what it must leave untouched and unread."""
import numpy as np
import pytest
import torch

from tests import emit_ref as R

pytestmark = pytest.mark.gpu

BEHIND = 1.0e30          # what the rows hold behind n_in in the shared launch; the second launch puts NaN there


def _launch(table, behind, order=None, mono_stride=None, hot=R.HOT_ROW):
    """One launch over the table (in `order`) plus, behind it, an fp32 mono twin of every int16 clip.  Returns per table clip the
    destination, per int16 clip its twin's, the buffers and every destination of the launch."""
    rows = R.make_rows(table, behind, hot=hot)
    dests, bufs = R.lay_out(table, mono_stride=mono_stride)
    twins = {}
    cursor = 0
    twin_buf = torch.full((sum(t[5] + 7 for t in table if t[3] == "i16") + 7,), R.SENTINEL_F32, dtype=torch.float32, device="cuda")
    for j, t in enumerate(table):
        if t[3] == "i16":
            twins[j] = R.Dest(twin_buf, cursor + 3, 0, 1, 1, t[5])
            cursor += t[5] + 7
    order = list(range(len(table))) if order is None else order
    jobs = [(j, dests[j]) for j in order] + [(j, twins[j]) for j in order if j in twins]
    R.emit([rows[j] for j, _d in jobs], [table[j][4] for j, _d in jobs], [table[j][0] for j, _d in jobs], [d for _j, d in jobs],
           [R.limit_of(j, hot) for j, _d in jobs])
    return rows, dests, twins, bufs, twin_buf


@pytest.fixture(scope="module")
def table():
    rows, dests, twins, bufs, twin_buf = _launch(R.CLIPS, BEHIND, mono_stride={6: 2})
    want = [R.composition(rows[j, :t[4]], t[0], t[3], R.limit_of(j)) for j, t in enumerate(R.CLIPS)]
    return rows, dests, twins, bufs, twin_buf, want


def _check(table, rows, dests, twins, bufs, twin_buf, want, what, hot=R.HOT_ROW):
    for j, ((rate, ch, layout, kind, n_in, n_out), d, w) in enumerate(zip(table, dests, want)):
        assert n_out == R.out_length(rate, n_in) and w.shape == (n_out,) and d.channels == ch
        got = d.read()
        assert w.dtype == got.dtype
        for c in range(ch):                                  # (1, 2, 3) the composition's bits, on both channels
            assert torch.equal(got[c], w), (what, j, rate, layout, kind, c, int((got[c] != w).sum()))
        f32 = twins[j].read()[0] if kind == "i16" else got[0]
        if kind == "i16":                                    # (2) numpy on the launch's own fp32 twin
            assert np.array_equal(got[0].cpu().numpy(), R.pcm16_numpy(f32.cpu().numpy(), R.limit_of(j, hot))), (what, j)
        y, bound = R.ref64(rows[j, :n_in].cpu().numpy(), rate)                                       # (5) float64
        err = np.abs(f32.cpu().numpy().astype(np.float64) - y)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"emit {what} clip {j} ({rate} Hz, {layout}, {kind}): n_out {n_out}, max err / bound {worst:.3f}")
        assert bool((err <= bound).all()), (what, j, worst)
    # (4) nothing outside the clips' spans was written
    assert R.untouched(bufs["f32"], dests, R.SENTINEL_F32), what
    assert R.untouched(bufs["i16"], dests, R.SENTINEL_I16), what
    assert R.untouched(twin_buf, list(twins.values()), R.SENTINEL_F32), what


def test_one_launch_is_the_composition_of_each_clip_alone(table):
    rows, dests, twins, bufs, twin_buf, want = table
    assert [R.out_length(t[0], t[4]) for t in R.CLIPS] == [6000, 6433, 5000, 55146, 4098, 1838, 117, 2, 1285]
    # both alignments of an int16 pair and of an interleaved frame, and the mono clip on every second slot
    assert [d.off % 2 for d, t in zip(dests, R.CLIPS) if t[3] == "i16"] == [0, 1, 0, 1] and dests[6].ss == 2
    hot = twins[R.HOT_ROW].read()[0]
    assert float(hot.max()) > R.HOT_LIMIT and float(hot.min()) < -R.HOT_LIMIT        # the clamp is hit, on both sides
    assert int(dests[R.HOT_ROW].read().max()) == 8192 and int(dests[R.HOT_ROW].read().min()) == -8192
    _check(R.CLIPS, rows, dests, twins, bufs, twin_buf, want, "table")


def test_what_lies_behind_n_in_changes_no_output_bit(table):
    _rows, dests, twins, bufs, twin_buf, _want = table
    _rows2, dests2, twins2, bufs2, twin_buf2 = _launch(R.CLIPS, float("nan"), mono_stride={6: 2})
    for k in ("f32", "i16"):
        assert torch.equal(bufs[k], bufs2[k]), k              # (every byte: a NaN that was read would show)
    assert torch.equal(twin_buf, twin_buf2)


def test_block_edges():
    rows, dests, twins, bufs, twin_buf = _launch(R.EDGES, BEHIND, hot=-1)
    assert [R.out_length(t[0], t[4]) for t in R.EDGES] == [256, 257, 257, 256]
    want = [R.composition(rows[j, :t[4]], t[0], t[3], R.LIMIT) for j, t in enumerate(R.EDGES)]
    _check(R.EDGES, rows, dests, twins, bufs, twin_buf, want, "edges", hot=-1)


def test_a_permutation_of_the_clips_permutes_the_outputs(table):
    _rows, dests, twins, _bufs, _twin_buf, _want = table
    perm = [5, 2, 7, 0, 8, 3, 6, 1, 4]
    _rows2, pdests, ptwins, pbufs, ptwin_buf = _launch(R.CLIPS, BEHIND, order=perm, mono_stride={6: 2})
    for j in range(len(R.CLIPS)):
        assert torch.equal(pdests[j].read(), dests[j].read()), j
    for j in twins:
        assert torch.equal(ptwins[j].read(), twins[j].read()), j
    assert R.untouched(pbufs["f32"], pdests, R.SENTINEL_F32) and R.untouched(pbufs["i16"], pdests, R.SENTINEL_I16)


def test_strided_destinations_are_descriptors_not_copies():
    """A (T, C) view over planar storage, a planar int16 pair whose second channel starts on the odd half of a word, interleaved
    fp32 frames on and off an 8-byte boundary, every third slot of a longer tensor."""
    n_in, rate = 3001, 16000
    n_out = R.out_length(rate, n_in)
    assert n_out == 2001
    row = R.make_rows([(rate, 1, "mono", "f32", n_in, n_out)], BEHIND, seed=90, hot=-1)[0]
    want = {"f32": R.composition(row[:n_in], rate), "i16": R.composition(row[:n_in], rate, "i16", 0.125)}
    sent = {"f32": R.SENTINEL_F32, "i16": R.SENTINEL_I16}
    dests = []
    for kind, dtype in (("f32", torch.float32), ("i16", torch.int16)):
        planar = torch.full((2, n_out), sent[kind], dtype=dtype, device="cuda")          # odd n_out: channel 1 starts on an odd element
        dests.append((kind, R.Dest.of_view(planar.t(), channels_last=True), planar))
        for shift in (0, 1):
            inter = torch.full((2 * n_out + 8,), sent[kind], dtype=dtype, device="cuda")
            dests.append((kind, R.Dest.of_view(inter[2 + shift:2 + shift + 2 * n_out].view(n_out, 2), channels_last=True), inter))
        third = torch.full((3 * n_out + 4,), sent[kind], dtype=dtype, device="cuda")
        dests.append((kind, R.Dest.of_view(third[1:1 + 3 * n_out].view(n_out, 3)[:, :1], channels_last=True), third))
    assert dests[0][1].cs == n_out and dests[0][1].ss == 1 and dests[3][1].ss == 3
    B = len(dests)
    R.emit([row] * B, [n_in] * B, [rate] * B, [d for _k, d, _b in dests], [0.125] * B)
    for kind, d, buf in dests:
        got = d.read()
        for c in range(d.channels):
            assert torch.equal(got[c], want[kind]), (kind, d.cs, d.ss, d.off, c)
        assert R.untouched(d.buf, [d], sent[kind]), (kind, d.cs, d.ss, d.off)
    assert int(want["i16"].max()) == 4096                    # limit 0.125 was hit


def test_more_clips_than_travel_as_kernel_arguments():
    """Up to 64 descriptors go with the launch, more are uploaded through the workspace: 70 short clips in one launch equal the
    same clips in launches of 35, and each its composition."""
    rates, n = [16000, 24000, 44100, 8000, 48000], 70
    table = [(rates[j % 5], 1 + j % 2, "interleaved" if j % 2 else "mono", "i16" if j % 3 else "f32", 250 + 3 * j,
              R.out_length(rates[j % 5], 250 + 3 * j)) for j in range(n)]
    rows = R.make_rows(table, BEHIND, seed=200, hot=-1)
    n_in, rate = [t[4] for t in table], [t[0] for t in table]
    dests, bufs = R.lay_out(table)
    R.emit(list(rows), n_in, rate, dests, [R.LIMIT] * n)
    dests2, bufs2 = R.lay_out(table)
    for part in (slice(0, 35), slice(35, 70)):
        R.emit(list(rows[part]), n_in[part], rate[part], dests2[part], [R.LIMIT] * 35)
    for k in ("f32", "i16"):
        assert torch.equal(bufs[k], bufs2[k]), k              # (sentinels included)
        assert R.untouched(bufs[k], dests, R.SENTINEL_F32 if k == "f32" else R.SENTINEL_I16)
    for j in (0, 1, 33, 64, 65, 69):
        want = R.composition(rows[j, :n_in[j]], rate[j], table[j][3])
        assert all(torch.equal(ch, want) for ch in dests[j].read()), j


def test_equal_rates_on_every_alignment():
    """An equal-rate clip takes wider blocks (2048 samples, four per thread, vector loads and stores where the alignment allows):
    one source row, off and on a 16-byte boundary, to every layout and sample type at each of the eight element offsets of a
    16-byte word, with a length that crosses the block and the round and ends on a partial group of four."""
    n = 4101
    table = [(R.CODEC_RATE, 1, "mono", "f32", n, n)]
    rows = R.make_rows(table * 2, BEHIND, seed=300, hot=-1)
    rows[1, 1:n + 1] = rows[0, :n]                           # the same samples one element off the boundary
    want = {"f32": R.composition(rows[0, :n], R.CODEC_RATE), "i16": R.composition(rows[0, :n], R.CODEC_RATE, "i16", 0.125)}
    assert int(want["i16"].max()) == 4096 and torch.equal(want["f32"], rows[0, :n])
    jobs = [(src, ch, layout, kind) for src in (0, 1) for kind in ("f32", "i16")
            for ch, layout in ((1, "mono"), (2, "interleaved"), (2, "planar"))]
    srcs, dests, bufs = [], [], []
    for src, ch, layout, kind in jobs:
        for shift in range(8):
            cs, ss, span = R.strides(layout, n)
            buf = torch.full((span + 24,), R.SENTINEL_F32 if kind == "f32" else R.SENTINEL_I16,
                             dtype=torch.float32 if kind == "f32" else torch.int16, device="cuda")
            srcs.append(rows[0] if src == 0 else rows[1, 1:])
            dests.append(R.Dest(buf, 8 + shift, cs, ss, ch, n))
            bufs.append((buf, kind))
    B = len(dests)
    assert B == 96                                           # (more than travel as kernel arguments: the uploaded form)
    R.emit(srcs, [n] * B, [R.CODEC_RATE] * B, dests, [0.125] * B)
    half = B // 2
    again = [R.Dest(torch.full_like(d.buf, -1), d.off, d.cs, d.ss, d.channels, n) for d in dests[half:]]      # the argument-block form
    R.emit(srcs[half:], [n] * half, [R.CODEC_RATE] * half, again, [0.125] * half)
    for d, d2 in zip(dests[half:], again):
        assert torch.equal(d.read(), d2.read()) and R.untouched(d2.buf, [d2], -1), (d.cs, d.ss, d.off)
    for d, (buf, kind) in zip(dests, bufs):
        got = d.read()
        for c in range(d.channels):
            assert torch.equal(got[c], want[kind]), (kind, d.cs, d.ss, d.off, c)
        assert R.untouched(buf, [d], R.SENTINEL_F32 if kind == "f32" else R.SENTINEL_I16), (kind, d.cs, d.ss, d.off)
