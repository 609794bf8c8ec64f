"""Batch invariance per kernel, across every launch form a batch size can select ("a dataset tokenised file
by file must equal the one tokenised in batches").  The pattern is the same everywhere: a small block of rows (70: no multiple
of 16, across a 64-row tile edge) or one clip with fixed contents is run alone, then again embedded among unrelated filler in
larger problems that differ only in batch extent (M, clips, nz): at offset 0, at an offset 128 k + 37 inside a later tile, and
flush with the end.  Its output must be the SAME WORDS as in the solo run: raw integer views (int32 for fp32, the int16 halves
for S32, both arrays of the dual formats), so NaN payloads and the sign of zero count.  There is no tolerance anywhere in this
file; the float64 bounds are the business of the per-kernel suites.

Operands are drawn once at the largest extent and sliced; row-indexed operands (the residual, the EPI_BIAS_ROW bias, the second
K source) travel with the block, column-indexed ones (weight with its scale, bias, gamma) stay fixed (tests/inv_ref.py).
Everything goes through the probes the per-kernel suites use; every case records the form the launcher reports, and each
group ends with a test that the forms compared are all the forms the launcher can choose.  The extents come from the launchers'
own conditions and the device's CU count (inv_ref.form16 / form32 mirror them; the probe's report is checked against the mirror).
The last group is the encode call itself at 65 ... 128 clips, where the persistent LSTM changes form."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_ref as G
from tests import inv_ref as I
from tests.test_gemm_epilogues import EXPECT16, EXPECT16_HEAD, EXPECT32, conv

pytestmark = pytest.mark.gpu

# gemm16s.hip WT_GEMM16H_PAIRS: the pairs the one-product twin exists for
PAIRS16H = [(G.EPI_BIAS, G.OUT_F32), (G.EPI_BIAS_RES, G.OUT_F32), (G.EPI_BIAS, G.OUT_S32), (G.EPI_BIAS_ROW, G.OUT_S32),
            (G.EPI_SCALE, G.OUT_F32), (G.EPI_BIAS_GELU, G.OUT_S32), (G.EPI_BIAS_GAMMA_RES, G.OUT_F32), (G.EPI_HEAD, G.OUT_S32)]
SEEN = {}                        # (engine, "plain" | "head") -> forms compared with a solo run
GRIDS = {}                       # engine -> {"one-shot", "persistent"}
_FAM = {}
_id16 = lambda p: f"{G.EPI_NAMES[p[0]]}-{G.OUT_NAMES[p[1]]}"


def _family(key, make):
    if key not in _FAM:
        _FAM[key] = make()
    return _FAM[key]


class _Group:
    """Runs of one problem family: the first is the solo run, every later one is compared with it."""

    def __init__(self, engine, epi, out, kind, what):
        self.engine, self.epi, self.out, self.kind, self.what = engine, epi, out, kind, what
        self.solo = None

    def __call__(self, runner, expect=None, **kw):
        form, res = runner(self.engine, self.epi, self.out, **kw)
        name = I.form_name(form)
        if expect is not None:
            assert name == expect, f"{self.what} {kw}: the launcher reports {name}, its conditions give {expect}"
        SEEN.setdefault((self.engine, self.kind), set()).add(name)
        GRIDS.setdefault(self.engine, set()).add("persistent" if form.G < form.tiles else "one-shot")
        if self.solo is None:
            self.solo = res[0]
        I.compare_blocks(self.solo, res, self.out, f"engine {self.engine} {self.what} {kw} on {name}")
        return form


def _lin_extents(N, K, nz, cus, table):
    """[(M, form)] of a family: the extents worked out for 256 CUs where the launcher's rule agrees on this device."""
    pick = lambda M: I.form16(M, N, K, nz, cus)
    return [(I.extent_for(pick, want, first), want) for first, want in table]


T192 = [(70, "64x32ks2p2"), (2000, "128x32ks2p1"), (4000, "128x64ks2p1"), (4352, "128x128"), (11521, "128x192")]
T160 = [(70, "128x32"), (2000, "128x64"), (4352, "128x128"), (11521, "128x192")]


def _plain_pair(engine, epi, out):
    cus = I.ncu()
    # ---- K = 192 (six K tiles: the KS = 2 forms are eligible), N = 384
    e192 = _lin_extents(384, 192, 1, cus, T192)
    m_max = max(M for M, _f in e192)
    fam = _family(("lin", 384, 192), lambda: I.LinFamily(384, 192, m_max, 2, seed=192))
    g = _Group(engine, epi, out, "plain", "K=192 N=384")
    for M, want in e192:
        g(fam.run, expect=want, M=M, offs=I.positions(M))
    # ... the same rows again beside a second z slice: M = 2000 then runs plain 128x64, which ties the KS = 1 and KS = 2 loops
    m64 = I.extent_for(lambda M: I.form16(M, 384, 192, 2, cus), "128x64", 2000)
    for M in (70, m64, e192[3][0]):
        g(fam.run, expect=I.form16(M, 384, 192, 2, cus), M=M, nz=2, offs=I.positions(M))
    # ---- a second K source: K1 = 96 is an odd number of K tiles, so the switch falls inside a KS = 2 pair
    g = _Group(engine, epi, out, "plain", "K=192 K1=96 N=384")
    for M, want in e192[:2]:
        g(fam.run, expect=want, M=M, offs=I.positions(M), K1=96)
    # ---- K = 160 (five K tiles: no KS = 2)
    e160 = _lin_extents(384, 160, 1, cus, T160)
    fam = _family(("lin", 384, 160), lambda: I.LinFamily(384, 160, max(M for M, _f in e160), 1, seed=160))
    g = _Group(engine, epi, out, "plain", "K=160 N=384")
    for M, want in e160:
        g(fam.run, expect=want, M=M, offs=I.positions(M))
    # ---- N = 64: 256x64 only.  K = 96 is too shallow for the persistent grid (it needs K / 32 >= stages + 1 = 4), so the
    #      one-shot extents run at K = 96 and at K = 128, and the persistent grid (G < tiles) at K = 128, reached as
    #      test_gemm_epilogues._cases16 reaches it: nz slices that leave 8 slots per slice, A shared, B an activation
    fam = _family(("lin", 64, 96), lambda: I.LinFamily(64, 96, 300, 1, seed=96))
    g = _Group(engine, epi, out, "plain", "K=96 N=64")
    for M in (70, 300):
        g(fam.run, expect="256x64", M=M, offs=I.positions(M))
    pz, mp = max(2, cus // 8), 256 * 9 + 7
    fam = _family(("lin", 64, 128), lambda: I.LinFamily(64, 128, mp, pz, seed=128, shared=True))
    g = _Group(engine, epi, out, "plain", "K=128 N=64 B=activation")
    for M, nz in ((70, 1), (300, 1), (mp, pz)):
        f = g(fam.run, expect="256x64", M=M, nz=nz, offs=I.positions(M), b_act=True)
    assert f.G < f.tiles, (f.G, f.tiles)
    # ---- conv gathers: the block is one clip; T_out = 25 and 40, so tiles straddle clips.  Alone, in each slot of three clips
    #      (a neighbour's samples must not reach it through the gather), and in the first, a middle and the last slot of a clip
    #      count that selects another tile form
    for tag, case_of in (("conv k=4 stride 2 reflect tap pairs", lambda n: conv(n, 50, 32, 96, 4, stride=2, tap_pair=True)),
                         ("conv k=5 dilation 2 zero pad", lambda n: conv(n, 40, 32, 96, 5, dil=2, pad_mode=0))):
        c1 = case_of(1)
        pick = lambda n: I.form16(n * c1.T_out, c1.N, c1.K, 1, cus, taps=c1.k)
        many = next(n for n in range(4, 4000) if pick(n) != pick(3))
        fam = _family(("conv", tag), lambda: I.ConvFamily(case_of, many, seed=c1.K))
        g = _Group(engine, epi, out, "plain", tag)
        g(fam.run, expect=pick(1), clips=1)
        for s in range(3):
            g(fam.run, expect=pick(3), clips=3, slots=(s,))
        g(fam.run, expect=pick(many), clips=many, slots=(0, many // 2, many - 1))


def _head_pair(engine):
    """The two forms of the head epilogue on one problem with N % 64 == 0."""
    cus = I.ncu()
    epi, out = G.EPI_HEAD, G.OUT_S32
    pick = lambda M: I.form16(M, 128, 192, 1, cus, head=True)
    big = I.extent_for(pick, "128x128", 1000)
    fam = _family(("head", 128, 192), lambda: I.LinFamily(128, 192, max(big, 1000), 1, seed=7, head=True))
    g = _Group(engine, epi, out, "head", "head K=192 N=128")
    for M in (70, 1000, big):
        g(fam.run, expect=pick(M), M=M, offs=I.positions(M))


@pytest.mark.parametrize("pair", G.PAIRS16, ids=_id16)
def test_gemm16s_rows_are_the_same_words_on_every_tile_form(pair):
    """Engine 0, the three-product kernel: "every tile shape accumulates K in the same order" (gemm16s.hip launch16s_tiled)."""
    if pair[0] == G.EPI_HEAD:
        _head_pair(0)
    else:
        _plain_pair(0, *pair)


@pytest.mark.parametrize("pair", PAIRS16H, ids=_id16)
def test_gemm16h_rows_are_the_same_words_on_every_tile_form(pair):
    """Engine 2, the one-product f16 twin, on the pairs it exists for."""
    if pair[0] == G.EPI_HEAD:
        _head_pair(2)
    else:
        _plain_pair(2, *pair)


def test_every_gemm16s_form_was_compared():
    """Runs after the two tests above: on both engines all eight non-head forms and both head forms were compared with a solo
    run on at least one problem, on a one-shot and on a persistent grid."""
    for engine in (0, 2):
        assert SEEN.get((engine, "plain")) == EXPECT16, (engine, SEEN.get((engine, "plain")))
        assert SEEN.get((engine, "head")) == EXPECT16_HEAD, (engine, SEEN.get((engine, "head")))
        assert GRIDS.get(engine) == {"one-shot", "persistent"}, (engine, GRIDS.get(engine))


# ================================================================================================ gemm.hip, engine 1 (fp32)
M32 = 128 * 257


@pytest.mark.parametrize("epi", [G.EPI_BIAS, G.EPI_BIAS_RES], ids=lambda e: G.EPI_NAMES[e])
@pytest.mark.parametrize("N", [96, 128, 32])
def test_gemm_fp32_rows_are_the_same_words_on_every_tile_form(N, epi):
    """The fp32 engine is the per-site fallback route after a range overflow.  N = 96: 128x64 alone, 128x96 at M = 128 * 257;
    N = 128: 128x64 alone, 128x128 at M = 128 * 257; N = 32: 128x32, placements only."""
    big = 300 if N == 32 else M32
    fam = _family(("lin32", N), lambda: I.LinFamily(N, 64, big, 1, seed=N))
    g = _Group(1, epi, G.OUT_F32, "plain", f"fp32 K=64 N={N}")
    for M in (70, big):
        g(fam.run, expect=I.form32(M, N), M=M, offs=I.positions(M))
    if N != 32:
        _FAM.pop(("lin32", N))               # 25 MB of filler, used by these two cases only


def test_every_fp32_form_was_compared():
    assert SEEN.get((1, "plain")) == EXPECT32, SEEN.get((1, "plain"))


# ================================================================================================ the vector quantiser
VQ_SEEN = set()


@pytest.mark.parametrize("kernel", [0, 1])
def test_vq_rows_are_the_same_words(kernel):
    """wt_vq_probe (row_sumsq, the distance GEMM with the argmax epilogue, vq_finalize) on the shipped codebook size: 70 rows
    alone, inside 1000 rows, and inside a row count whose tiles exceed gemm16s's persistent grid
    (test_vq_ops.test_more_tiles_than_workgroups).  Every partial candidate (value and index per part), the final codes and
    the feature words of the block."""
    from tests import vq_ref as V
    from tests.test_vq_ops import run_vq
    bins, D = 4096, 512
    gen = torch.Generator().manual_seed(40 + kernel)
    rows_big = 128 * (I.ncu() // -(-bins // V.geometry(0, bins)[0]) + 1) + 1
    embed = torch.randn(bins, D, generator=gen).float()
    block = torch.randn(I.BLOCK, D, generator=gen).float()
    fill = torch.randn(rows_big, D, generator=gen).float()
    _f, pv0, pi0, co0, ft0 = run_vq(block, embed, kernel, 1, I.BLOCK)
    assert bool(((co0 >= 0) & (co0 < bins)).all())
    I.assert_written(ft0, "the block's features")
    for rows in (1000, rows_big):
        offs = I.positions(rows)
        f, pv, pi, co, ft = run_vq(I.embed(fill[:rows], block, offs), embed, kernel, 1, rows)
        wrapped = f.grid < f.ntiles
        VQ_SEEN.add((kernel, wrapped))
        for o in offs:
            what = f"vq kernel {kernel}, {rows} rows, block at {o}"
            I.assert_same_words(I.words(pv[o:o + I.BLOCK]), I.words(pv0), what + ": partial values")
            I.assert_same_words(I.words(pi[o:o + I.BLOCK]), I.words(pi0), what + ": partial indices")
            I.assert_same_words(I.words(co[o:o + I.BLOCK]), I.words(co0), what + ": codes")
            I.assert_same_words(I.words(ft[0, :, o:o + I.BLOCK]), I.words(ft0[0]), what + ": features")


def test_every_vq_grid_was_compared():
    """gemm16s (kernel 0) one-shot and persistent; gemm.hip (kernel 1) has no persistent form."""
    assert VQ_SEEN == {(0, False), (0, True), (1, False)}, VQ_SEEN


# ================================================================================================ the fused encoder resblocks
RB_SEEN = set()
RB_SLOTS = (0, 2, 4)             # the clip sits in the first, a middle and the last slot of five; slots 1 and 3 hold filler


def _rb_batch(run, make, T_of):
    """run(B, T, inp) -> (form, words [B][rows][ch]); make(B, T, seed) -> inputs {name: [B][...]}; T_of(slots): a length whose
    tile count over five clips exceeds the resident workgroup slots (test_encoder_ops.test_resblock16_wrapped_grid)."""
    B = len(RB_SLOTS) + 2
    f0, _ = run(1, T_of(0, 1), make(1, T_of(0, 1), 0))
    slots = I.ncu() * min(4, 160 * 1024 // f0.lds)
    T = T_of(slots, B)
    clip, fill = make(1, T, 1), make(B, T, 2)
    fs, solo = run(1, T, clip)
    fb, many = run(B, T, {k: I.embed(fill[k], clip[k], RB_SLOTS) for k in clip})
    assert (fs.kernel, fs.C, fs.fold, fs.down, fs.fpw) == (fb.kernel, fb.C, fb.fold, fb.down, fb.fpw)
    assert fs.grid == fs.tiles and fb.grid < fb.tiles, (fs.grid, fs.tiles, fb.grid, fb.tiles)
    I.assert_written(solo, "the clip alone")
    RB_SEEN.add((fb.kernel, fb.C, fb.fold, fb.down, fb.fpw))
    return solo, many, fb


@pytest.mark.parametrize("fp32_chain", [0, 1], ids=["split-f16", "fp32-chain"])
@pytest.mark.parametrize("form", ["c32_fold", "c32_plain", "c64"])
def test_resblock_clip_is_the_same_words_in_any_slot(form, fp32_chain):
    from tests import test_encoder_ops as T
    arch, stage, C, _fold, _fpw, valid = T.FORMS[form]
    _W, D = T.weights(arch, stage)
    rows = (128 if C == 32 else 64) if fp32_chain else valid
    make = lambda B, Tn, seed: T.inputs(form, B, Tn, 1000 * seed + C)
    for elu_out, out_s32 in ((0, 0),) if fp32_chain else ((1, 1), (0, 0)):
        run = lambda B, Tn, inp: T.run_rb(D, B, Tn, C, elu_out=elu_out, out_s32=out_s32, fp32_chain=fp32_chain, **inp)
        solo, many, _f = _rb_batch(run, make, lambda slots, B: rows * (slots // B + 2) - 5)
        for s in RB_SLOTS:
            I.assert_same_words(I.words(many[s], out_s32), I.words(solo[0], out_s32), f"resblock {form} fp32={fp32_chain} elu={elu_out} s32={out_s32} slot {s}",
                                s32=bool(out_s32))


@pytest.mark.parametrize("r", [4, 2])
def test_resblock_down_clip_is_the_same_words_in_any_slot(r):
    from tests import test_encoder_ops as T
    _W, D = T.weights(T.DOWN[r], 1)
    opt = (126 - 2 * r) // r + 1
    make = lambda B, Tn, seed: dict(wav=torch.randn(B, Tn, generator=torch.Generator().manual_seed(10 * seed + r)).float().double())
    run = lambda B, Tn, inp: T.run_rb(D, B, Tn, 32, r=r, **inp)
    solo, many, _f = _rb_batch(run, make, lambda slots, B: max(1024, opt * r * (slots // B + 2) - 3))
    for s in RB_SLOTS:
        I.assert_same_words(I.words(many[s]), I.words(solo[0]), f"resblock down r={r} slot {s}")


def test_every_resblock_form_was_compared():
    """The instantiations launch_resblock16, launch_resblock16_down and launch_resblock can pick
    (test_encoder_ops.test_every_instantiation_was_reached), each alone on a one-shot grid against a wrapped grid."""
    want = {(0, 32, 1, 0, 32), (0, 32, 0, 0, 32), (0, 64, 0, 0, 16), (0, 32, 1, 4, 32), (0, 32, 1, 2, 32),
            (2, 32, 1, 0, 32), (2, 32, 0, 0, 32), (2, 64, 0, 0, 32)}
    assert RB_SEEN == want, RB_SEEN ^ want


# ================================================================================================ per-clip decoder ops
OPS_SEEN = set()
OP_B, OP_SLOT = 5, 3


def _dev(t):
    return t.float().contiguous().cuda()


def _clip_alone_and_in_slot(run, s32=False, what=""):
    """run(clip indices) -> (form name, output words per clip [len(indices)][...]): slot 3 of five clips against the clip alone."""
    n5, many = run(list(range(OP_B)))
    n1, one = run([OP_SLOT])
    OPS_SEEN.update((n5, n1))
    I.assert_written(one[0], what)
    I.assert_same_words(I.words(many[OP_SLOT], s32), I.words(one[0], s32), f"{what} ({n1} alone, {n5} in a batch)", s32=s32)


@pytest.mark.parametrize("T", [4, 257])
def test_conv_first_clip(T):
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(T)
    wav, w, b = torch.randn(OP_B, T, generator=gen), _dev(torch.randn(7, 32, generator=gen)), _dev(torch.randn(32, generator=gen))

    def run(idx):
        x, y = _dev(wav[idx]), I.nan_out(len(idx) * T * 32)
        name = I.op_probe(_capi.WT_OP_CONV_FIRST, B=len(idx), L=T, k=7, Cout=32, x=x.data_ptr(), p0=w.data_ptr(), p1=b.data_ptr(), y=y.data_ptr())
        return name, y.reshape(len(idx), -1)
    _clip_alone_and_in_slot(run, what=f"conv_first T={T}")


@pytest.mark.parametrize("Cin,k", [(32, 7), (64, 3)], ids=["conv_last32", "conv_last"])
@pytest.mark.parametrize("T", [4, 257])
def test_conv_last_clip(T, Cin, k):
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(T + Cin)
    xs, w = torch.randn(OP_B, T, Cin, generator=gen), _dev(torch.randn(k, Cin, generator=gen) / (k * Cin) ** 0.5)
    b = _dev(torch.tensor([0.3, 0.0, 0.0, 0.0]))

    def run(idx):
        x, y = _dev(xs[idx]), I.nan_out(len(idx) * T)
        name = I.op_probe(_capi.WT_OP_CONV_LAST, B=len(idx), L=T, C=Cin, k=k, flag=1, x=x.data_ptr(), p0=w.data_ptr(), p1=b.data_ptr(), y=y.data_ptr())
        assert name == ("conv_last32" if (Cin, k) == (32, 7) else "conv_last")
        return name, y.reshape(len(idx), -1)
    _clip_alone_and_in_slot(run, what=f"conv_last T={T} Cin={Cin}")


@pytest.mark.parametrize("T", [4, 257])
def test_convtr_clip(T):
    from wavtokenizer_amd import _capi
    Cin, Cout, stride = 64, 32, 4
    gen = torch.Generator().manual_seed(T)
    xs = torch.randn(OP_B, T, Cin, generator=gen)
    w, b = _dev(torch.randn(2 * stride, Cin, Cout, generator=gen) / (2 * Cin) ** 0.5), _dev(torch.randn(Cout, generator=gen))

    def run(idx):
        x, y = _dev(xs[idx]), I.nan_out(len(idx) * T * stride * Cout)
        name = I.op_probe(_capi.WT_OP_CONVTR, B=len(idx), L=T, C=Cin, Cout=Cout, k=2 * stride, stride=stride, flag=1, x=x.data_ptr(),
                          p0=w.data_ptr(), p1=b.data_ptr(), y=y.data_ptr())
        return name, y.reshape(len(idx), -1)
    _clip_alone_and_in_slot(run, what=f"convtr T={T}")


@pytest.mark.parametrize("mode,L,C,s32", [(0, 7, 768, 0), (0, 50, 256, 1), (0, 411, 256, 0), (1, 7, 768, 1), (1, 50, 256, 0), (2, 7, 768, 0), (2, 50, 256, 1)])
def test_rownorm_clip(mode, L, C, s32):
    """dwconv + LayerNorm (mode 0: both kernels, 5 x 411 rows are past the 2048 of its one-row form), LayerNorm (1), and the
    GroupNorm-apply + LayerNorm form (2) whose input scale and shift are per clip and travel with it."""
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(17 * mode + L + C)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    xs = rnd(OP_B, L, C)
    os_, oh = _dev(rnd(C) * 0.5 + 1), _dev(rnd(C))
    dw_w, dw_b = (_dev(rnd(7, C) / 7 ** 0.5), _dev(rnd(C))) if mode == 0 else (None, None)
    isc, ish = (torch.rand(OP_B, C, generator=gen) + 0.5, rnd(OP_B, C)) if mode == 2 else (None, None)
    p = lambda t: None if t is None else t.data_ptr()

    def run(idx):
        B = len(idx)
        x, y = _dev(xs[idx]), I.nan_out(B * L * C)
        sc, sh = (_dev(isc[idx]), _dev(ish[idx])) if mode == 2 else (None, None)
        status = torch.zeros(4, dtype=torch.int32, device="cuda")
        name = I.op_probe(_capi.WT_OP_ROWNORM, mode=mode, B=B, L=L, C=C, eps=1e-6, out_s32=s32, x=x.data_ptr(), p0=p(dw_w), p1=p(dw_b),
                          p2=p(sc), p3=p(sh), p4=os_.data_ptr(), p5=oh.data_ptr(), y=y.data_ptr(), status=status.data_ptr())
        assert int(status[0]) == 0
        return name, y.reshape(B, -1)
    _clip_alone_and_in_slot(run, s32=bool(s32), what=f"rownorm mode {mode} L={L} C={C}")


@pytest.mark.parametrize("L,ld,s32,mis", [(31, 32, 0, 0), (250, 256, 1, 0), (31, 32, 1, 1), (9, 10, 0, 0)],
                         ids=["reg", "reg-s32", "rmw-misaligned-s32", "rmw-pitch-10"])
def test_softmax_clip(L, ld, s32, mis):
    """Seven score rows per clip, in place (and the S32 copy): the register kernel and the read-modify-write kernel."""
    from wavtokenizer_amd import _capi
    from tests.test_decoder_ops import _softmax_scores
    rows = 7
    s = _softmax_scores(OP_B * rows, L, torch.Generator().manual_seed(L + ld)).reshape(OP_B, rows, L)

    def run(idx):
        n = len(idx) * rows
        h = torch.full((n, ld), float("nan"))
        h[:, :L] = s[idx].reshape(n, L)
        S = torch.zeros(n * ld + 4, device="cuda")
        S[mis:mis + n * ld] = h.reshape(-1).cuda()
        P = I.nan_out(n * ld) if s32 else None
        name = I.op_probe(_capi.WT_OP_SOFTMAX, n=n, L=L, ld=ld, x=S.data_ptr() + 4 * mis, y=P.data_ptr() if s32 else None)
        assert name == ("softmax_rmw" if (mis or ld % 4) else "softmax_reg<1>"), name
        return name, (P if s32 else S[mis:mis + n * ld]).reshape(len(idx), -1)
    _clip_alone_and_in_slot(run, s32=bool(s32), what=f"softmax L={L} ld={ld}")


@pytest.mark.parametrize("center", [0, 1], ids=["plain", "center"])
def test_istft_ola_clip(center):
    from wavtokenizer_amd import _capi
    n_fft, hop, L = 1280, 320, 5
    Kq = (n_fft // 4 + 1 + 31) // 32 * 32
    parts = torch.randn(4, OP_B, L, Kq, generator=torch.Generator().manual_seed(center))
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64).float()
    wd, qd = _dev(win), _dev(win * win)
    T = hop * (L - 1 if center else L)

    def run(idx):
        x, y = _dev(parts[:, idx]), I.nan_out(len(idx) * T)
        name = I.op_probe(_capi.WT_OP_ISTFT_OLA, B=len(idx), L=L, n_fft=n_fft, hop=hop, Kq=Kq, flag=center, x=x.data_ptr(), p0=wd.data_ptr(),
                          p1=qd.data_ptr(), y=y.data_ptr())
        return name, y.reshape(len(idx), -1)
    _clip_alone_and_in_slot(run, what=f"istft_ola center={center}")


@pytest.mark.parametrize("R,C,s32", [(255, 33, 0), (32, 33, 1)])
def test_transpose_clip(R, C, s32):
    from wavtokenizer_amd import _capi
    xs = torch.randn(OP_B, R, C, generator=torch.Generator().manual_seed(R + C))

    def run(idx):
        x, y = _dev(xs[idx]), I.nan_out(len(idx) * R * C)
        status = torch.zeros(4, dtype=torch.int32, device="cuda")
        name = I.op_probe(_capi.WT_OP_TRANSPOSE, B=len(idx), L=R, C=C, out_s32=s32, x=x.data_ptr(), y=y.data_ptr(), status=status.data_ptr())
        return name, y.reshape(len(idx), -1)
    _clip_alone_and_in_slot(run, s32=bool(s32), what=f"transpose R={R} C={C}")


@pytest.mark.parametrize("s32", [0, 1])
def test_code_rows_clip(s32):
    from wavtokenizer_amd import _capi
    bins, C, K, L = 7, 64, 3, 5
    rng = np.random.default_rng(5)
    table = torch.from_numpy(rng.standard_normal((K * bins, C)).astype(np.float32)).cuda()
    codes = torch.from_numpy(rng.integers(0, bins, size=(K, OP_B, L), dtype=np.int64))

    def run(idx):
        B = len(idx)
        cd, y = codes[:, idx].contiguous().cuda(), I.nan_out(B * L * C)
        bad, status = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        name = I.op_probe(_capi.WT_OP_CODE_ROWS, B=B, L=L, C=C, k=K, n=bins, out_s32=s32, x=cd.data_ptr(), p0=table.data_ptr(), y=y.data_ptr(),
                          y2=bad.data_ptr(), status=status.data_ptr())
        assert int(bad[0]) == 0 and int(status[0]) == 0
        return name, y.reshape(B, -1)
    _clip_alone_and_in_slot(run, s32=bool(s32), what="code_rows")


def test_every_per_clip_op_was_compared():
    want = {"conv_first", "conv_last32", "conv_last", "convtr", "dwconv_ln<3,1>", "dwconv_ln<1,1>", "dwconv_ln<1,4>", "rownorm<3,1>", "rownorm<1,1>",
            "rownorm<3,2>", "rownorm<1,2>", "softmax_reg<1>", "softmax_rmw", "istft_ola", "transpose", "code_rows"}
    assert OPS_SEEN == want, OPS_SEEN ^ want


# ================================================================================================ the encode call, 65 ... 128 clips
_ENC = {}


def _encoder():
    if not _ENC:
        from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth
        arch = NAMED_ARCHS["hop600"]
        sd = synth.make_state_dict(arch, seed=321)
        m = WavTokenizer.from_arch(arch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        m = m.eval().to("cuda")
        m.set_graph_max_clips(0)
        _ENC["m"] = m
        _ENC["wav"] = torch.from_numpy(synth.make_clips(128, 24000, seed=3)).cuda()
        _ENC["solo"] = {}
    return _ENC["m"], _ENC["wav"], _ENC["solo"]


@pytest.mark.parametrize("B", [65, 100, 128])
def test_encode_call_is_batch_invariant_above_64_clips(B):
    """wt_encode on hop-600, 24 000 samples per clip, at batch sizes that run the persistent LSTM's BIG form (more than eight
    clips per XCD): the encoder output before quantisation and the codes of clips 0, B // 2 and B - 1 are the words of one-clip
    calls (the SMALL form).  Up to the parent of the commit that added this test the BIG form summed the split-f16 correction
    products in one interleaved chain and the SMALL form in two, and every B above 64 differed."""
    from wavtokenizer_amd import _capi
    pl = ctypes.c_int32()
    assert _capi.lib.wt_device_info(torch.cuda.current_device(), None, None, ctypes.byref(pl)) == 0
    if not pl.value:
        pytest.skip("wt_device_info reports no persistent LSTM on this device")
    m, wav, solo = _encoder()
    with torch.inference_mode():
        _f, codes, emb = m._run_encode(wav[:B], want_emb=True)
        for i in (0, B // 2, B - 1):
            if i not in solo:
                _f1, c1, e1 = m._run_encode(wav[i:i + 1], want_emb=True)
                solo[i] = (I.words(c1[:, 0]), I.words(e1[0]))
            I.assert_same_words(I.words(emb[i]), solo[i][1], f"encode B={B} clip {i}: emb_out")
            I.assert_same_words(I.words(codes[:, i]), solo[i][0], f"encode B={B} clip {i}: codes")
    assert m.persistent_lstm
    m.check_status()
