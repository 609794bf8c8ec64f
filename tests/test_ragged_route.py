"""The boundary between the two descriptor routes of the ragged calls (csrc/ragged.h launch_ragged): up to N clips travel in the
kernel's argument block and nothing is uploaded, N + 1 clips are uploaded into the head of the workspace.  The four families that
take both routes (wt_emit, wt_overlap_add_ragged and wt_mel_spectrogram / wt_mel_distance with N = 64, wt_stoi with N = 32), each
at B = N and B = N + 1, through the arenas of their own test modules:

  - every clip's output equals, bit for bit, that clip launched alone;
  - the canaries around the outputs are intact and nothing is written behind the workspace;
  - at B = N the descriptor region at the head of the workspace, filled with 0xAB beforehand, still holds the fill byte;
  - at B = N + 1 it does not.

The clips are the smallest that still span more than one block or frame.  The clips of B = N are the first N of B = N + 1, so the
launches of one clip alone are made once per family."""
import numpy as np
import pytest
import torch

from tests import emit_ref, mel_ref, stoi_ref
from tests.test_overlap_add_ragged_op import Launch, _recordings

pytestmark = pytest.mark.gpu

FILL = 0xAB


def _filled(ws):
    return bool((torch.as_tensor(ws) == FILL).all())


# ------------------------------------------------------------------------------------------------ wt_emit, N = 64
# (target rate, channels, layout, sample type, n_in): 257 to 260 outputs each, a resampling block holds 256; 24000 Hz is the copy form
EMIT_KINDS = [(16000, 1, "mono", "f32", 390), (22050, 2, "interleaved", "i16", 280), (24000, 1, "mono", "i16", 257),
              (44100, 2, "planar", "f32", 141), (24000, 2, "interleaved", "f32", 258)]


def _emit_launch(table, rows, which):
    """Clips `which` of the table in one launch into fresh destinations laid out for the whole table."""
    dests, bufs = emit_ref.lay_out(table)
    ws = emit_ref.emit([rows[j] for j in which], [table[j][4] for j in which], [table[j][0] for j in which], [dests[j] for j in which],
                       [emit_ref.limit_of(j, hot=-1) for j in which])
    return dests, bufs, ws


@pytest.fixture(scope="module")
def emit_alone():
    table = [k + (emit_ref.out_length(k[0], k[4]),) for k in (EMIT_KINDS[j % len(EMIT_KINDS)] for j in range(65))]
    assert all(256 < t[5] < 1000 for t in table)
    rows = emit_ref.make_rows(table, behind=float("nan"), hot=-1)
    alone = []
    for j in range(len(table)):
        dests, _bufs, _ws = _emit_launch(table, rows, [j])
        alone.append(dests[j].read())
    return table, rows, alone


@pytest.mark.parametrize("B", [64, 65])
def test_emit(emit_alone, B):
    table, rows, alone = emit_alone
    dests, bufs, (ws, behind) = _emit_launch(table[:B], rows, range(B))
    for j in range(B):
        assert torch.equal(dests[j].read(), alone[j]), (B, j, table[j])
    assert emit_ref.untouched(bufs["f32"], dests, emit_ref.SENTINEL_F32) and emit_ref.untouched(bufs["i16"], dests, emit_ref.SENTINEL_I16)
    assert _filled(behind)
    assert _filled(ws) == (B == 64)


# ------------------------------------------------------------------------------------------------ wt_overlap_add_ragged, N = 64
# (frame_len, stride, total): the last one crosses the 256-output block edges
OLA_CASES = [(8, 8, 8), (8, 6, 20), (8, 3, 17), (8, 1, 12), (257, 100, 999)]


@pytest.fixture(scope="module")
def ola_alone():
    recs = _recordings([OLA_CASES[j % len(OLA_CASES)] for j in range(65)], seed=400)
    alone = []
    for j, rec in enumerate(recs):
        one = Launch([rec], seed=500 + j)
        assert one.canaries_intact()
        alone.append(one.result(0))
    return recs, alone


@pytest.mark.parametrize("B", [64, 65])
def test_overlap_add_ragged(ola_alone, B):
    recs, alone = ola_alone
    run = Launch(recs[:B], seed=3)
    for j in range(B):
        assert np.array_equal(run.result(j), alone[j]), (B, j, recs[j][0])
    assert run.canaries_intact()
    assert _filled(run.behind_workspace)
    assert _filled(run.workspace) == (B == 64)


# ------------------------------------------------------------------------------------------------ wt_mel_*, N = 64
MEL_LENGTHS = (513, 600, 1300, 1025, 1291)      # 3 to 6 frames at hop 256: one block of four frames, or two


@pytest.fixture(scope="module")
def mel_alone():
    from wavtokenizer_amd._capi import lib
    a = [mel_ref.signal(mel_ref.BROADBAND[j % 4], MEL_LENGTHS[j % 5], seed=j) for j in range(65)]
    b = [mel_ref.signal("noise", len(x), seed=100 + j) for j, x in enumerate(a)]
    spec, dist = [], []
    for x, y in zip(a, b):
        (s,), ok = mel_ref.run([x])
        (d,), ok2 = mel_ref.run([x], [y])
        assert ok and ok2
        spec.append(s)
        dist.append(d)
    return a, b, spec, dist, lambda B: int(lib.wt_mel_workspace_bytes(B, 0))       # (no frames: the descriptor region alone)


@pytest.mark.parametrize("B", [64, 65])
def test_mel_spectrogram(mel_alone, B):
    a, _b, spec, _dist, desc_bytes = mel_alone
    got, intact, ws = mel_ref.run(a[:B], with_workspace=True)                     # (asserts that nothing is written behind the workspace)
    for j in range(B):
        assert np.array_equal(got[j], spec[j]), (B, j, len(a[j]))
    assert intact
    assert _filled(ws[:desc_bytes(B)]) == (B == 64)


@pytest.mark.parametrize("B", [64, 65])
def test_mel_distance(mel_alone, B):
    a, b, _spec, dist, desc_bytes = mel_alone
    got, intact, ws = mel_ref.run(a[:B], b[:B], with_workspace=True)
    assert np.array_equal(np.array(got, np.float32), np.array(dist[:B], np.float32)), B
    assert np.isfinite(got).all() and min(got) > 0
    assert intact
    assert _filled(ws[:desc_bytes(B)]) == (B == 64)
    assert not _filled(ws[desc_bytes(B):])                                        # (the per-frame partials behind the descriptors)


# ------------------------------------------------------------------------------------------------ wt_stoi, N = 32
STOI_T = 4097                                   # at 10 kHz: K0 = 31 candidate frames, all kept: 30 frames, one segment


@pytest.fixture(scope="module")
def stoi_alone():
    from wavtokenizer_amd._capi import lib
    clean = [stoi_ref.speechlike(STOI_T, stoi_ref.FS, seed=j) for j in range(33)]
    proc = [stoi_ref.noisy(x, 5.0 + j % 7, seed=j) for j, x in enumerate(clean)]
    assert stoi_ref.candidate_frames(STOI_T) == 31
    alone = {}
    for ext in (False, True):
        runs = [stoi_ref.run([x], [y], stoi_ref.FS, extended=ext, with_taps=False) for x, y in zip(clean, proc)]
        assert all(r.intact for r in runs)
        alone[ext] = np.array([r.d[0] for r in runs], np.float32)
        assert np.isfinite(alone[ext]).all() and (alone[ext] != np.float32(1e-5)).all()      # (a segment was there to measure)
    h = stoi_ref.handle(stoi_ref.FS)
    return clean, proc, alone, lambda B: int(lib.wt_stoi_workspace_bytes(h, B, 0, 0)) - 8 * B     # (less the (K0, K) pair per clip)


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("B", [32, 33])
def test_stoi(stoi_alone, B, extended):
    clean, proc, alone, desc_bytes = stoi_alone
    r = stoi_ref.run(clean[:B], proc[:B], stoi_ref.FS, extended=extended, with_taps=False)
    assert np.array_equal(r.d, alone[extended][:B]), (B, extended)
    assert r.intact                                                                # (canaries and the bytes behind the workspace)
    assert _filled(r.ws[:desc_bytes(B)]) == (B == 32)
