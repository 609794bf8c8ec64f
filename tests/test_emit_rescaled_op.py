"""The rescaling emit alone (csrc/audio.hip emit_level_kernel, wt_emit_rescaled): per clip the bits of wt_pcm16 with rescale = 1
on the clip's own wt_emit fp32 output (int16), or that output times min(limit / max |output|, 1) (fp32), for the equal-rate copy
and two resampled rates, every layout and store form, block-edge lengths, batches of 1 and 65, clips under the limit, far over
it and silent, with guard words around every destination.

n_out runs over 1, 2, 255, 256, 257 and 2049 at the codec rate and at 16 kHz; 24 000 -> 44 100 Hz cannot produce every length
(n_out = ceil(147 n_in / 80) skips values), so there each target is replaced by the next length that exists."""
import pytest
import torch

from tests import emit_ref as R
from tests import level_ref as LR

pytestmark = pytest.mark.gpu

RATES = [24000, 16000, 44100]
TARGETS = [1, 2, 255, 256, 257, 2049]
LAYOUTS = [(1, "mono"), (2, "planar"), (2, "interleaved")]
LEVELS = ["under", "over", "under", "over", "silent"]        # under: peak below the limit (scale 1, no clamp); over: 20 x that
BEHIND = 1.0e30


def _n_in_for(rate, target):
    """(n_in, n_out): the shortest clip whose length at `rate` is the first one >= target that exists."""
    n_in = max(1, target * R.CODEC_RATE // rate - 2)
    while R.out_length(rate, n_in) < target:
        n_in += 1
    return n_in, R.out_length(rate, n_in)


def _table():
    """(rate, channels, layout, sample type, n_in, n_out, level) per clip: every rate x target length, then every rate x layout x
    sample type at 1500 samples; layouts, sample types and levels take turns."""
    t = []
    for rate in RATES:
        for target in TARGETS:
            n_in, n_out = _n_in_for(rate, target)
            ch, layout = LAYOUTS[len(t) % 3]
            t.append((rate, ch, layout, ("i16", "f32")[(len(t) // 3) % 2], n_in, n_out, LEVELS[len(t) % 5]))
    for rate in RATES:
        for ch, layout in LAYOUTS:
            for kind in ("i16", "f32"):
                t.append((rate, ch, layout, kind, 1500, R.out_length(rate, 1500), LEVELS[len(t) % 5]))
    return t


def _rows(table, seed=40):
    """The source rows [B][pitch] on the GPU, BEHIND past each clip's n_in; make_clips stays within about +-0.4."""
    rows = R.make_rows([t[:6] for t in table], BEHIND, seed=seed, hot=-1)
    for j, t in enumerate(table):
        if t[6] == "over":
            rows[j, :t[4]] *= 20.0
        elif t[6] == "silent":
            rows[j, :t[4]] = 0.0
    return rows


def _limit(j):
    return (0.99, 0.5, 0.25)[j % 3]


def _run(table, rows, emit_dests=None):
    """wt_emit_rescaled over the table and wt_emit of every clip to an fp32 mono twin; returns (dests, bufs, twins, twin buffers)."""
    dests, bufs = R.lay_out([t[:6] for t in table]) if emit_dests is None else emit_dests
    mono = [(t[0], 1, "mono", "f32", t[4], t[5]) for t in table]
    twins, twin_bufs = R.lay_out(mono)
    B = len(table)
    n_in, rates, limits = [t[4] for t in table], [t[0] for t in table], [_limit(j) for j in range(B)]
    R.emit(list(rows), n_in, rates, twins, limits)
    LR.emit_rescaled(list(rows), n_in, rates, dests, limits)
    return dests, bufs, twins, twin_bufs


def _want(twin, kind, limit):
    """The composition on a clip's own fp32 output: wt_pcm16 with rescale = 1, or the fp32 product."""
    from wavtokenizer_amd import audio
    f32 = twin.read()[0].contiguous()
    if kind == "i16":
        return audio.to_pcm16(f32, rescale=True, limit=limit)
    return f32 * LR.rescale_factor(f32, limit)


def _check(table, dests, bufs, twins, what):
    seen = set()
    for j, (t, d, tw) in enumerate(zip(table, dests, twins)):
        want = _want(tw, t[3], _limit(j))
        got = d.read()
        assert got.dtype == want.dtype and got.shape == (t[1], t[5])
        for c in range(t[1]):
            assert torch.equal(got[c], want), (what, j, t, c, int((got[c] != want).sum()))
        peak = float(tw.read().abs().max())
        seen.add("silent" if peak == 0 else "under" if peak < _limit(j) else "over")
        if t[3] == "i16" and peak >= _limit(j):                                   # the loudest sample sits at the limit, not beyond it
            assert int(got.abs().max()) == int(torch.round(torch.tensor(_limit(j) * 32768.0)))
        if t[3] == "f32" and 0 < peak < _limit(j):                                # scale 1: the fp32 output itself
            assert torch.equal(got[0], tw.read()[0])
    assert R.untouched(bufs["f32"], dests, R.SENTINEL_F32), what                 # guard words before, between and behind the clips
    assert R.untouched(bufs["i16"], dests, R.SENTINEL_I16), what
    return seen


@pytest.fixture(scope="module")
def table():
    t = _table()
    return t, _rows(t)


def test_one_launch_is_the_composition_of_each_clip_alone(table):
    t, rows = table
    assert len(t) == 36 and [x[5] for x in t[:12]] == [1, 2, 255, 256, 257, 2049] * 2
    assert [x[5] for x in t[12:18]] == [2, 2, 256, 256, 258, 2049]                # what 44 100 Hz has at or above the targets
    dests, bufs, twins, _tb = _run(t, rows)
    assert _check(t, dests, bufs, twins, "table") == {"silent", "under", "over"}
    for lay in ("mono", "planar", "interleaved"):                                 # every rate x layout x sample type was there
        for kind in ("i16", "f32"):
            assert {x[0] for x in t if x[2] == lay and x[3] == kind} == set(RATES)


def test_batches_of_one_and_of_65(table):
    t, rows = table
    for j in (5, 11, 17, 20):                                                     # one clip per launch
        dests, bufs, twins, _tb = _run([t[j]], rows[j:j + 1])
        want = _want(twins[0], t[j][3], _limit(0))
        assert all(torch.equal(ch, want) for ch in dests[0].read()), j
        assert R.untouched(bufs["f32"], dests, R.SENTINEL_F32) and R.untouched(bufs["i16"], dests, R.SENTINEL_I16)
    big = (t + t)[:65]                                                            # beyond the 64 descriptors of the argument block
    big_rows = torch.cat([rows, rows])[:65]
    dests, bufs, twins, _tb = _run(big, big_rows)
    _check(big, dests, bufs, twins, "65 clips")


def test_every_int16_alignment_and_strided_destinations():
    """int16 runs starting at each of the four 2-byte alignments within 8 bytes (and the four behind them), planar and interleaved
    pairs alike, at the equal rate (wide copy blocks) and resampled; a mono clip on every third slot, a (T, C) view of planar
    storage and interleaved frames off their natural boundary, both sample types."""
    from wavtokenizer_amd import audio
    limit = 0.5
    for rate in (24000, 16000):
        n_in, n = _n_in_for(rate, 2049)
        row = _rows([(rate, 1, "mono", "f32", n_in, n, "over")], seed=77)[0]
        f32 = audio.convert_audio(row[None, None, :n_in].clone(), R.CODEC_RATE, rate, 1)[0, 0]
        want = {"i16": audio.to_pcm16(f32, rescale=True, limit=limit), "f32": f32 * LR.rescale_factor(f32, limit)}
        assert float(f32.abs().max()) > 2 * limit and int(want["i16"].abs().max()) == 16384
        jobs = []
        for kind, dtype, sent in (("i16", torch.int16, R.SENTINEL_I16), ("f32", torch.float32, R.SENTINEL_F32)):
            for ch, layout in LAYOUTS:
                for shift in range(8):
                    cs, ss, span = R.strides(layout, n)
                    buf = torch.full((span + 24,), sent, dtype=dtype, device="cuda")
                    jobs.append((kind, R.Dest(buf, 8 + shift, cs, ss, ch, n), sent))
            planar = torch.full((2, n), sent, dtype=dtype, device="cuda")            # odd n: channel 1 starts on an odd element
            jobs.append((kind, R.Dest.of_view(planar.t(), channels_last=True), sent))
            third = torch.full((3 * n + 4,), sent, dtype=dtype, device="cuda")
            jobs.append((kind, R.Dest.of_view(third[1:1 + 3 * n].view(n, 3)[:, :1], channels_last=True), sent))
        B = len(jobs)
        assert B == 52
        LR.emit_rescaled([row] * B, [n_in] * B, [rate] * B, [d for _k, d, _s in jobs], [limit] * B)
        for kind, d, sent in jobs:
            got = d.read()
            for c in range(d.channels):
                assert torch.equal(got[c], want[kind]), (rate, kind, d.cs, d.ss, d.off, c)
            assert R.untouched(d.buf, [d], sent), (rate, kind, d.cs, d.ss, d.off)


def test_the_limit_is_checked_for_both_sample_types():
    from wavtokenizer_amd import _capi
    t = [(16000, 1, "mono", "f32", 300, 200, "under")]
    rows = _rows(t)
    dests, bufs = R.lay_out([x[:6] for x in t])
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(_capi.WavTokError) as e:
            LR.emit_rescaled(list(rows), [300], [16000], dests, [bad])
        assert e.value.status == _capi.WT_ERR_INVALID and "limit" in str(e.value)
    assert R.untouched(bufs["f32"], [], R.SENTINEL_F32)
