"""The ragged ingest kernel (csrc/audio.hip ingest_kernel, wt_ingest) alone: one launch over clips of eight rates, both
channel counts, both layouts and both sample types against audio.convert_audio of each clip alone (bit for bit), against a
float64 evaluation of the polyphase sum (derived bound, tests/ingest_ref.py), and for what it must leave untouched; and the
ragged way out, wt_codes_unpack."""
import numpy as np
import pytest
import torch

from tests import ingest_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


@pytest.fixture(scope="module")
def model():
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    return WavTokenizer.from_arch(ARCH_HOP600).to("cuda")      # (no weights: the ingest needs the model's staging alone)


def _place(clips, gpu_odd):
    """Half of the clips on the GPU, half on the CPU (they travel through the pinned buffer)."""
    return [c.cuda() if (i % 2 == 1) == gpu_odd else c for i, c in enumerate(clips)]


def _composition(clip, rate, layout):
    from wavtokenizer_amd import audio
    return audio.convert_audio(R.planar_f32(clip.cuda(), layout).contiguous()[None], rate, R.CODEC_RATE)[0, 0]


@pytest.fixture(scope="module")
def table(model):
    """The eight clips, one launch with a pitch beyond the longest clip, and each clip's composition."""
    rows = R.table_clips()
    clips, rates, layouts = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    T_pad = max(R.out_length(sr, n) for sr, _c, _l, _k, n in R.CLIPS) + 77
    out, n_out = R.ingest(model, _place(clips, True), rates, layouts, T_pad=T_pad, sentinel=SENTINEL)
    want = [_composition(c, sr, lay) for c, sr, lay in rows]
    return rows, out, n_out, want


def _check_rows(rows, out, n_out, want, what):
    for j, ((clip, rate, layout), n, w) in enumerate(zip(rows, n_out, want)):
        assert w.shape == (n,) and n == R.out_length(rate, R.planar_f32(clip, layout).shape[1])
        assert torch.equal(out[j, :n], w), (what, j, rate, float((out[j, :n] - w).abs().max()))      # (i) the composition's bits
        assert bool((out[j, n:] == SENTINEL).all()), (what, j)                                       # (ii) nothing past n_out
        y, bound = R.ref64(R.planar_f32(clip, layout).numpy(), rate)                                 # (iv) float64
        err = np.abs(out[j, :n].cpu().numpy().astype(np.float64) - y)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"ingest {what} clip {j} ({rate} Hz, {layout}, {clip.dtype}): n_out {n}, max err / bound {worst:.3f}")
        assert bool((err <= bound).all()), (what, j, worst)


def test_rows_are_convert_audio_of_each_clip_alone(table):
    rows, out, n_out, want = table
    assert n_out == [13500, 7621, 5000, 16333, 1025, 8708, 1050, 1]
    _check_rows(rows, out, n_out, want, "table")


def test_block_edges(model):
    rows = R.table_clips(R.EDGE_N_IN)
    clips, rates, layouts = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    out, n_out = R.ingest(model, _place(clips, False), rates, layouts, T_pad=512, sentinel=SENTINEL)
    assert n_out == [383, 279, 257, 80]
    _check_rows(rows, out, n_out, [_composition(*r) for r in rows], "edges")


def test_a_permutation_of_the_clips_permutes_the_rows(model, table):
    rows, out, n_out, _want = table
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    prow = [rows[i] for i in perm]
    pout, pn = R.ingest(model, _place([r[0] for r in prow], False), [r[1] for r in prow], [r[2] for r in prow],
                        T_pad=out.shape[1], sentinel=SENTINEL)
    assert pn == [n_out[i] for i in perm]
    assert torch.equal(pout, out[perm])                      # (sentinels included)


def test_opposite_channels_cancel_exactly(model):
    left = R.make_clip(44100, 1, "mono", "i16", 3000, seed=5)
    inter = torch.stack([left, -left], dim=1)                # (T, 2) int16 (no sample is -32768: the clips stay below 0.5)
    assert int(left.min()) > -32768
    planar = torch.stack([left, -left], dim=0).float() / 32768
    out, n_out = R.ingest(model, [inter, planar.cuda()], [44100, 22050], ["interleaved", "planar"], sentinel=SENTINEL)
    for j, n in enumerate(n_out):
        assert bool((out[j, :n] == 0).all()), j
    assert bool((out[0, n_out[0]:] == SENTINEL).all())


def test_strided_views_are_descriptors_not_copies(model):
    """A device clip is read through its own strides: every second sample of a longer tensor, and a (T, C) view of a planar one."""
    base = R.make_clip(16000, 2, "planar", "f32", 4001, seed=9).cuda()
    every_other = base[:, ::2]                               # (2, 2001), sample stride 2
    as_tc = base.t()                                         # (4001, 2) view: channels_last over planar storage
    out, n_out = R.ingest(model, [every_other, as_tc], [16000, 16000], ["planar", "interleaved"], sentinel=SENTINEL)
    assert torch.equal(out[0, :n_out[0]], _composition(every_other.contiguous(), 16000, "planar"))
    assert torch.equal(out[1, :n_out[1]], _composition(base, 16000, "planar"))


def test_codes_unpack_copies_each_rows_span():
    from wavtokenizer_amd import _capi
    B, L_pad = 5, 300
    codes = torch.arange(B * L_pad, dtype=torch.int64, device="cuda").view(1, B, L_pad)
    L = [300, 1, 0, 257, 256]
    order = [3, 0, 4, 1, 2]                                  # rows land in another order than they sit in the batch
    offs, pos = [0] * B, 0
    for b in order:
        offs[b], pos = pos, pos + L[b]
    # two more rows that must be skipped whole: a span longer than the row, a span that runs past the flat tensor
    codes7 = torch.cat([codes, codes[:, :2]], dim=1).contiguous()
    spans = torch.tensor([[L[b], offs[b]] for b in range(B)] + [[L_pad + 1, 0], [10, pos + 5 - 9]], dtype=torch.int64).cuda()
    flat = torch.full((pos + 5,), -9, dtype=torch.int64, device="cuda")
    _capi.check(_capi.lib.wt_codes_unpack(codes7.data_ptr(), B + 2, L_pad, spans.data_ptr(), flat.data_ptr(), flat.numel(),
                                          torch.cuda.current_stream().cuda_stream), "wt_codes_unpack")
    torch.cuda.synchronize()
    for b in range(B):
        assert torch.equal(flat[offs[b]:offs[b] + L[b]], codes[0, b, :L[b]]), b
    assert bool((flat[pos:] == -9).all())
