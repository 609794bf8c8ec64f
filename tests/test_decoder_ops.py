"""Every non-GEMM kernel of csrc/ops.hip alone, one launch at a time through wt_op_probe (the plans' own launchers), against
the float64 references of tests/op_ref.py.  Per case: (a) the launch form the launcher reports is the one the case is named
for; (b) every element within its derived bound, all finite (gemm_ref.check: no sampling, no outliers allowed); (c) the guard
words before and after every output untouched, owned pad regions exactly zero; (d) bit equality between forms where the
code promises it.  The last test compares the (kernel, variant) pairs the session reached with the ones the launchers can
pick.  tests/test_op_checks.py holds the CPU half: the bounds pass an honest fp32 evaluation and reject the slips."""
import ctypes

import pytest
import torch

from tests import gemm_ref as G
from tests import op_ref as O
from tests import parity_log

pytestmark = pytest.mark.gpu

GUARD = 64                       # fp32 words of sentinel before and after every output
SENT = -559038737                # 0xDEADBEEF
HIT = set()                      # form names reached in this session
WORST = {}                       # op -> worst |got - ref| / bound


class Out:
    """A device output of n fp32 words between two guard runs, pre-filled with NaN (every logical element must be written)."""

    def __init__(self, n, fill_nan=True):
        self.n = n
        h = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32)
        if fill_nan:
            h[GUARD:GUARD + n] = 0x7FC00000
        self.buf = h.cuda()
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def host(self):
        h = self.buf.cpu()
        assert bool((h[:GUARD] == SENT).all()) and bool((h[GUARD + self.n:] == SENT).all()), "guard words overwritten"
        return h[GUARD:GUARD + self.n]

    def f32(self):
        return self.host().view(torch.float32)

    def i16(self):
        return self.host().view(torch.int16)


def _dev(t):
    return None if t is None else t.float().contiguous().cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def probe(op, **kw):
    """One wt_op_probe call; returns the form name (kernel<variant[,variant2]>) and the raw form."""
    from wavtokenizer_amd import _capi
    d = _capi.WtOpDesc()
    d.size = ctypes.sizeof(d)
    d.op = op
    for k, v in kw.items():
        setattr(d, k, v)
    f = _capi.WtOpForm()
    rc = _capi.lib.wt_op_probe(ctypes.byref(d), ctypes.byref(f), None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    k = _capi.WT_OPK_NAMES[f.kernel]
    if k in ("gn_tile", "dwconv_ln", "rownorm"):
        name = f"{k}<{f.variant},{f.variant2}>"
    elif k in ("gn_chunk", "gn_stats", "softmax_reg"):
        name = f"{k}<{f.variant}>"
    else:
        name = k
    HIT.add(name)
    return name, f


def _check(op, got, ref, bound, what=""):
    nbad, frac, finite = G.check(got, ref, bound)
    WORST[op] = max(WORST.get(op, 0.0), frac if finite else float("inf"))
    assert finite, f"{what}: an element was not written or is not finite"
    assert nbad == 0, f"{what}: {nbad} elements outside the bound (worst {frac:.3g} x bound)"
    return frac


def family(name, shape, gen, axis_group=None):
    """Input families: x of `shape`; statistics are taken over groups of the last axis described by the caller, the
    families only need to be hard for any of them."""
    x = torch.randn(*shape, generator=gen)
    if name in ("normal", "swishwide"):
        return x
    if name == "mean100":
        return x + 100.0
    if name == "const":                  # everything constant: every group / row has variance 0
        return torch.full(shape, 3.0)
    if name == "spike":
        x = x * 1e-3
        x.reshape(-1)[:: max(1, x.numel() // 7) + 1] = 1e4
        return x
    if name == "tiny":
        return x * 1e-20
    if name == "huge":
        return x * 1e15
    if name == "small":                  # variance about eps = 1e-6
        return x * 1e-3
    if name == "wide":                   # activation arguments across [-100, 100]
        return (torch.rand(*shape, generator=gen) * 200 - 100)
    raise ValueError(name)


HARD = ["mean100", "const", "spike", "tiny", "huge", "small"]


# ================================================================================================ GroupNorm
def _gn_expect(C, groups, L, part, mode):
    """The form launch_gn_apply (mode 1 / 2) and launch_gn_stats (mode 0) pick, read from the launchers."""
    cg = C // groups
    GB = next((g for g in range(1, groups + 1) if groups % g == 0 and (g * cg) % 32 == 0 and g * cg <= 128), 0)
    slab = GB and cg % 4 == 0 and C % 4 == 0 and GB <= 8
    if mode == 0:
        return "gn_chunk<0>" if (part and L > 256 and slab) else "gn_stats<0>"
    if slab and L * GB * cg * 4 <= 96 * 1024:
        nt = 512 if GB == 4 else 256
        return f"gn_tile<{mode - 1},{2 if nt // 64 == 2 * GB else 1}>"
    if part and slab:
        return f"gn_chunk<{mode}>"
    return f"gn_stats<{mode}>"


def _run_gn(B, L, C, groups, fam, swish, s32, part, seed, apply=True, x=None):
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(seed)
    if x is None:
        x = family(fam, (B, L, C), gen).float()
    gamma = (torch.rand(C, generator=gen) + 0.5).float()
    beta = torch.randn(C, generator=gen).float()
    if fam == "swishwide":               # activation arguments across [-100, 100] (where exp(-v) overflows, and beyond)
        beta = torch.linspace(-100, 100, C).float()
    ref = O.groupnorm(x.double(), gamma.double(), beta.double(), groups, 1e-6, act=bool(swish), out_s32=bool(s32))
    xd, gd, bd = _dev(x), _dev(gamma), _dev(beta)
    y, sc, sh = Out(B * L * C), Out(B * C), Out(B * C)
    nch = (L + 127) // 128
    pt = torch.zeros(B * groups * nch * 2, device="cuda") if part else None
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    kw = dict(B=B, L=L, C=C, groups=groups, eps=1e-6, x=_p(xd), p0=_p(gd), p1=_p(bd), p2=_p(pt), y2=sc.ptr, y3=sh.ptr,
              status=_p(status))
    if apply:
        name, f = probe(_capi.WT_OP_GN_APPLY, flag=swish, out_s32=s32, y=y.ptr, **kw)
    else:
        name, f = probe(_capi.WT_OP_GN_STATS, **kw)
    want = _gn_expect(C, groups, L, part, (2 if swish else 1) if apply else 0)
    assert name == want, (name, want)
    what = f"gn B{B} L{L} C{C} {fam} {name}"
    op = "gn_apply" if apply else "gn_stats"
    _check(op, sc.f32().reshape(B, C), *ref["scale"], what + " scale")
    _check(op, sh.f32().reshape(B, C), *ref["shift"], what + " shift")
    bits = None
    if apply:
        if s32:
            bits = y.i16()
            got = G.decode_s32_rows(bits, B * L, C).reshape(B, L, C)
        else:
            bits = y.host()
            got = bits.view(torch.float32).reshape(B, L, C)
        _check(op, got, *ref["y"], what)
        assert int(status[0]) == 0
    else:
        y.host()                 # untouched, guards included
    return bits, f


GN_L = [1, 2, 3, 7, 120, 121, 127, 128, 129, 255, 256, 257, 385, 777, 1200, 1281]
GN_CASES = ([(B, L, 768, 32, "normal", (i + B) & 1, ((i + B) >> 1) & 1, True) for i, L in enumerate(GN_L) for B in (1, 3)]
            + [(64, 120, 768, 32, "normal", 1, 1, True)]
            + [(2, L, 768, 32, fam, sw, 0, True) for L in (7, 255, 256, 385) for fam in HARD for sw in (0, 1)]
            + [(2, L, C, 32, fam, sw, s32, True) for C in (256, 512, 1024) for L, fam, sw, s32 in
               ((1, "normal", 1, 0), (121, "normal", 0, 1), (255, "mean100", 1, 0), (768, "normal", 1, 1), (769, "normal", 0, 0),
                (900, "spike", 1, 1))]
            + [(2, 120, 768, 32, "swishwide", 1, 0, True), (2, 385, 768, 32, "swishwide", 1, 0, True), (2, 130, 96, 32, "swishwide", 1, 0, True)]
            # geometries that fall through to gn_stats_kernel<1|2>: 3 channels per group; no chunk scratch above L = 256
            + [(2, L, 96, 32, fam, sw, s32, True) for L, fam, sw, s32 in ((5, "normal", 0, 0), (300, "mean100", 1, 0), (130, "normal", 1, 1),
                                                                         (64, "const", 0, 1))]
            + [(2, L, 768, 32, fam, sw, s32, False) for L, fam, sw, s32 in ((257, "normal", 0, 0), (1281, "normal", 1, 1), (385, "mean100", 1, 0),
                                                                          (300, "const", 0, 0))])


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: "B{}-L{}-C{}-g{}-{}-sw{}-s32{}-part{}".format(*c))
def test_gn_apply(case):
    B, L, C, groups, fam, sw, s32, part = case
    _run_gn(B, L, C, groups, fam, sw, s32, part, seed=L * 7 + C + B)


@pytest.mark.parametrize("case", [(2, L, 768, fam, part) for L, fam, part in
                                  ((1, "normal", True), (255, "mean100", True), (256, "normal", True), (257, "normal", True),
                                   (257, "normal", False), (777, "spike", True), (1281, "const", True), (385, "huge", True),
                                   (385, "tiny", True))]
                         + [(3, 300, 512, "normal", True), (2, 40, 96, "normal", True)],
                         ids=lambda c: "B{}-L{}-C{}-{}-part{}".format(*c))
def test_gn_stats(case):
    """The statistics-only call: gn_stats_kernel<0> up to L = 256 (and without scratch), the chunked pair above."""
    B, L, C, fam, part = case
    _run_gn(B, L, C, 32, fam, 0, 0, part, seed=L + C, apply=False)


@pytest.mark.parametrize("L,C,part,s32", [(120, 768, True, 0), (256, 768, True, 1), (385, 768, True, 0), (1200, 768, True, 1),
                                          (300, 768, False, 0), (200, 512, True, 0), (100, 96, True, 0)])
def test_gn_clip_bits_do_not_depend_on_the_batch(L, C, part, s32):
    """'a clip's statistics are summed in the same order whatever the batch': clip 1 of a batch of 3 alone gives the same bits."""
    gen = torch.Generator().manual_seed(L + C)
    x = torch.randn(3, L, C, generator=gen)
    many, _ = _run_gn(3, L, C, 32, "normal", 1, s32, part, seed=5, x=x)
    one, _ = _run_gn(1, L, C, 32, "normal", 1, s32, part, seed=5, x=x[1:2].clone())
    per = many.numel() // 3
    assert torch.equal(many[per:2 * per], one)


# ================================================================================================== row norms
def _run_rownorm(mode, B, L, C, fam, s32, seed, x=None):
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(seed)
    if x is None:
        x = family(fam, (B, L, C), gen).float()
    os_, oh = (torch.randn(C, generator=gen) * 0.5 + 1).float(), torch.randn(C, generator=gen).float()
    dw_w = (torch.randn(7, C, generator=gen) / 7 ** 0.5).float() if mode == 0 else None
    dw_b = torch.randn(C, generator=gen).float() if mode == 0 else None
    isc = (torch.rand(B, C, generator=gen) + 0.5).float() if mode == 2 else None
    ish = torch.randn(B, C, generator=gen).float() if mode == 2 else None
    dbl = lambda t: None if t is None else t.double()
    ref, bound = O.rownorm(mode, x.double(), os_.double(), oh.double(), 1e-6, dbl(dw_w), dbl(dw_b), dbl(isc), dbl(ish), out_s32=bool(s32))
    t = [_dev(v) for v in (x, dw_w, dw_b, isc, ish, os_, oh)]
    y = Out(B * L * C)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    name, f = probe(_capi.WT_OP_ROWNORM, mode=mode, B=B, L=L, C=C, eps=1e-6, out_s32=s32, x=_p(t[0]), p0=_p(t[1]), p1=_p(t[2]),
                    p2=_p(t[3]), p3=_p(t[4]), p4=_p(t[5]), p5=_p(t[6]), y=y.ptr, status=_p(status))
    NV = C // 256
    want = f"dwconv_ln<{NV},{1 if B * L <= 2048 else 4}>" if mode == 0 else f"rownorm<{NV},{mode}>"
    assert name == want, (name, want)
    if mode == 0:
        waves = B * L if B * L <= 2048 else B * ((L + 3) // 4)
        assert f.grid_x == (waves + 3) // 4 and f.block == 256
    bits = y.i16() if s32 else y.host()
    got = G.decode_s32_rows(bits, B * L, C).reshape(B, L, C) if s32 else bits.view(torch.float32).reshape(B, L, C)
    _check("rownorm", got, ref, bound, f"rownorm mode{mode} B{B} L{L} C{C} {fam} {name}")
    assert int(status[0]) == 0
    return bits


# (B, L): B L in {1, 2047, 2048, 2049}; L % 4 in {0, 1, 2, 3} in the R = 4 form; L in {1, 2, 3, 4, 6, 7} in both forms, B >= 2
RN_BL = [(1, 1), (23, 89), (2, 1024), (8, 256), (3, 683), (3, 684), (3, 685), (3, 686), (2, 1), (2, 2), (2, 3), (2, 4), (2, 6), (2, 7),
         (2049, 1), (1025, 2), (700, 3), (600, 4), (400, 6), (300, 7)]
RN_CASES = ([(0, B, L, 768, "normal", i & 1) for i, (B, L) in enumerate(RN_BL)]
            + [(m, B, L, 768, "normal", i & 1) for m in (1, 2) for i, (B, L) in enumerate(((1, 1), (2, 7), (3, 683), (23, 89)))]
            + [(m, 3, 50, 768, fam, 0) for m in (0, 1, 2) for fam in HARD]
            + [(m, B, L, C, fam, s32) for C in (256, 512, 1024) for m, B, L, fam, s32 in
               ((0, 2, 5, "normal", 0), (0, 3, 685, "normal", 1), (0, 300, 7, "mean100", 0), (1, 3, 50, "normal", 1), (1, 2, 3, "spike", 0),
                (2, 3, 50, "normal", 0), (2, 2, 130, "mean100", 1))])


@pytest.mark.parametrize("case", RN_CASES, ids=lambda c: "mode{}-B{}-L{}-C{}-{}-s32{}".format(*c))
def test_rownorm(case):
    mode, B, L, C, fam, s32 = case
    _run_rownorm(mode, B, L, C, fam, s32, seed=17 * mode + B + L + C)


@pytest.mark.parametrize("C", [256, 512, 768, 1024])
def test_dwconv_ln_forms_give_the_same_bits(C):
    """'Same accumulation order per output as rownorm_kernel, so the results are identical': clip 0 of a batch that takes
    dwconv_ln<NV, 4> (B L > 2048, L % 4 = 3) has the bits of the same clip alone through dwconv_ln<NV, 1>."""
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(3, 703, C, generator=gen)
    r4 = _run_rownorm(0, 3, 703, C, "normal", 0, seed=9, x=x)
    r1 = _run_rownorm(0, 1, 703, C, "normal", 0, seed=9, x=x[:1].clone())
    assert torch.equal(r4[:703 * C], r1)


# ==================================================================================================== softmax
def _softmax_scores(rows, L, gen):
    """Rows of every family: spreads 0 (all equal), 1 and 200, the maximum in column 0 and in column L - 1."""
    s = torch.randn(rows, L, generator=gen)
    for r in range(rows):
        k = r % 7
        if k == 1:
            s[r] = 0.37
        elif k == 2:
            s[r] = torch.rand(L, generator=gen)
        elif k in (3, 4):
            s[r] = torch.rand(L, generator=gen) * 200 - 200
            s[r, 0 if k == 3 else L - 1] = 0.5
        elif k == 5:
            s[r, L - 1] = 9.0
        elif k == 6:
            s[r, 0] = 9.0
    return s.float()


def _run_softmax(rows, L, ld, s32, misalign, seed, s=None):
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(seed)
    if s is None:
        s = _softmax_scores(rows, L, gen)
    ref, bound = O.softmax(s.double(), out_s32=bool(s32))
    S = Out(rows * ld + 4)
    h = torch.full((rows, ld), float("nan"))          # pad columns on entry: NaN, in odd rows a huge finite value
    h[1::2] = 3e38
    h[:, :L] = s
    off = 1 if misalign else 0
    S.buf[GUARD + off:GUARD + off + rows * ld] = h.reshape(-1).view(torch.int32).cuda()
    if off:
        S.buf[GUARD] = SENT
    S.buf[GUARD + off + rows * ld:GUARD + rows * ld + 4] = SENT
    P = Out(rows * ld) if s32 else None
    name, f = probe(_capi.WT_OP_SOFTMAX, n=rows, L=L, ld=ld, x=S.ptr + 4 * off, y=P.ptr if s32 else None)
    nv = 1 if ld <= 256 else 2 if ld <= 512 else 5 if ld <= 1280 else 8
    want = "softmax_rmw" if (misalign or ld > 2048 or ld % 4) else f"softmax_reg<{nv}>"
    assert name == want, (name, want)
    assert f.grid_x == (rows + 3) // 4
    sh = S.host()
    assert int(sh[0]) == SENT or not off
    assert bool((sh[off + rows * ld:] == SENT).all()), "words after the score matrix overwritten"
    if s32:
        bits = P.i16()
        full = G.decode_s32_rows(bits, rows, ld)
        assert bool((bits.reshape(rows, -1, 2, 32).permute(0, 1, 3, 2).reshape(rows, ld, 2)[:, L:] == 0).all()), "S32 pad columns not zero"
    else:
        bits = sh[off:off + rows * ld]
        full = bits.view(torch.float32).reshape(rows, ld).double()
        assert bool((bits.reshape(rows, ld)[:, L:] == 0).all()), "pad columns not exactly zero"
    got = full[:, :L]
    _check("softmax", got, ref, bound, f"softmax rows{rows} L{L} ld{ld} {name}")
    dev = (got.sum(-1) - 1).abs().max().item()
    assert dev <= L * O.ULP, f"row sums off by {dev:.3g} > L ULP"
    return bits


SM_PITCH = [32, 256, 288, 512, 544, 1280, 1312, 2048, 2080]
SM_CASES = [(13 if i & 1 else 7, L, ld, (i + j) & 1, 0) for i, ld in enumerate(SM_PITCH) for j, L in enumerate((ld, ld - 1, ld - 31))]
SM_CASES += [(9, L, ld, s32, 1) for ld, L, s32 in ((32, 5, 0), (256, 255, 1), (544, 513, 0), (1312, 1300, 1), (2048, 2047, 0))]
SM_CASES += [(6, 9, 10, 0, 0), (1, 1, 32, 1, 0), (3, 1, 4, 0, 0)]          # a pitch that is no multiple of 4; one column


@pytest.mark.parametrize("case", SM_CASES, ids=lambda c: "rows{}-L{}-ld{}-s32{}-mis{}".format(*c))
def test_softmax(case):
    rows, L, ld, s32, mis = case
    _run_softmax(rows, L, ld, s32, mis, seed=L + ld)


@pytest.mark.parametrize("L,ld,s32", [(31, 32, 0), (250, 256, 1), (500, 512, 0), (1200, 1216, 1), (2000, 2048, 0), (1500, 1504, 1)])
def test_softmax_forms_give_the_same_bits(L, ld, s32):
    """'Same arithmetic per element (max, exp(x - max), sum in the same lane order, division by the sum)': the register
    kernel and the read-modify-write kernel (forced by a base 4 bytes off alignment) agree bit for bit."""
    s = _softmax_scores(10, L, torch.Generator().manual_seed(L))
    a = _run_softmax(10, L, ld, s32, 0, seed=1, s=s)
    b = _run_softmax(10, L, ld, s32, 1, seed=1, s=s)
    assert torch.equal(a, b)


# ================================================================================================== ISTFT tail
def _istft_chunks(B, L, hop, center):
    return -(-(B * hop * (L - 1 if center else L)) // 256)


IS_CASES = [(n_fft, hop, c, B, L) for n_fft, hop in ((2400, 600), (1280, 320)) for c in (0, 1)
            for B, L in ((1, 1), (3, 2), (2, 3), (8, 4), (3, 5), (2, 120), (1, 777)) if not (c and L == 1)]
IS_CASES += [(1280, 320, 0, 4, 120), (1280, 320, 1, 8, 5)]             # chunk counts that are multiples of 8 before rounding


def test_istft_case_table_covers_both_chunk_roundings():
    m8 = {_istft_chunks(B, L, hop, c) % 8 == 0 for _n, hop, c, B, L in IS_CASES}
    assert m8 == {True, False}


@pytest.mark.parametrize("case", IS_CASES, ids=lambda c: "nfft{}-hop{}-center{}-B{}-L{}".format(*c))
def test_istft_ola(case):
    from wavtokenizer_amd import _capi
    n_fft, hop, center, B, L = case
    Q = n_fft // 4
    Kq = (Q + 1 + 31) // 32 * 32
    gen = torch.Generator().manual_seed(n_fft + 10 * L + B)
    parts = torch.randn(4, B, L, Kq, generator=gen).float()
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64).float()
    wsq = (win * win).float()
    ref, bound = O.istft_tail(parts.double(), win.double(), n_fft, hop, bool(center))
    T = ref.shape[-1]
    assert T == hop * (L - 1 if center else L)
    pd, wd, qd = _dev(parts), _dev(win), _dev(wsq)
    y = Out(B * T)
    name, f = probe(_capi.WT_OP_ISTFT_OLA, B=B, L=L, n_fft=n_fft, hop=hop, Kq=Kq, flag=center, x=_p(pd), p0=_p(wd), p1=_p(qd), y=y.ptr)
    assert name == "istft_ola"
    assert f.grid_x == (_istft_chunks(B, L, hop, center) + 7) // 8 * 8 and f.block == 256
    _check("istft_ola", y.f32().reshape(B, T), ref, bound, f"istft {case}")


# ================================================================================================= small convs
T_LIST = [1, 2, 3, 4, 255, 256, 257, 1000]


@pytest.mark.parametrize("T", T_LIST)
def test_conv_first(T):
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(T)
    B, k, Cout = 3, 7, 32
    wav = torch.randn(B, T, generator=gen).float()
    w = (torch.randn(k, Cout, generator=gen) / k ** 0.5).float()
    bias = torch.randn(Cout, generator=gen).float()
    ref, bound = O.conv_first(wav.double(), w.double(), bias.double())
    xd, wd, bd = _dev(wav), _dev(w), _dev(bias)
    y = Out(B * T * Cout)
    name, _f = probe(_capi.WT_OP_CONV_FIRST, B=B, L=T, k=k, Cout=Cout, x=_p(xd), p0=_p(wd), p1=_p(bd), y=y.ptr)
    assert name == "conv_first"
    _check("conv_first", y.f32().reshape(B, T, Cout), ref, bound, f"conv_first T{T}")


@pytest.mark.parametrize("T", T_LIST)
@pytest.mark.parametrize("Cin,k,elu_in,fam", [(32, 7, 1, "normal"), (32, 7, 0, "normal"), (32, 7, 1, "wide"), (16, 7, 1, "wide"),
                                              (64, 3, 0, "normal"), (32, 5, 1, "normal"), (4, 7, 1, "normal"), (256, 7, 0, "normal")])
def test_conv_last(Cin, k, elu_in, fam, T):
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(T + Cin + k)
    B = 3
    x = family(fam, (B, T, Cin), gen).float()
    w = (torch.randn(k, Cin, generator=gen) / (k * Cin) ** 0.5).float()
    bias = torch.randn(1, generator=gen).float()
    ref, bound = O.conv_last(x.double(), w.double(), bias.double(), bool(elu_in))
    xd, wd = _dev(x), _dev(w)
    bd = torch.zeros(4, device="cuda")
    bd[0] = bias[0]
    y = Out(B * T)
    name, _f = probe(_capi.WT_OP_CONV_LAST, B=B, L=T, C=Cin, k=k, flag=elu_in, x=_p(xd), p0=_p(wd), p1=_p(bd), y=y.ptr)
    assert name == ("conv_last32" if (Cin, k) == (32, 7) else "conv_last")
    _check("conv_last", y.f32().reshape(B, T), ref, bound, f"{name} T{T} Cin{Cin} k{k} elu{elu_in} {fam}")


@pytest.mark.parametrize("T", T_LIST)
@pytest.mark.parametrize("Cin,Cout,stride,elu_in,fam", [(64, 32, 4, 1, "normal"), (32, 16, 2, 0, "normal"), (16, 8, 5, 1, "wide"), (8, 4, 8, 1, "normal")])
def test_convtr(Cin, Cout, stride, elu_in, fam, T):
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(T + Cin)
    B, k = 2, 2 * stride
    x = family(fam, (B, T, Cin), gen).float()
    w = (torch.randn(k, Cin, Cout, generator=gen) / (2 * Cin) ** 0.5).float()
    bias = torch.randn(Cout, generator=gen).float()
    ref, bound = O.convtr(x.double(), w.double(), bias.double(), stride, bool(elu_in))
    assert ref.shape == (B, T * stride, Cout)
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    y = Out(B * T * stride * Cout)
    name, _f = probe(_capi.WT_OP_CONVTR, B=B, L=T, C=Cin, Cout=Cout, k=k, stride=stride, flag=elu_in, x=_p(xd), p0=_p(wd), p1=_p(bd), y=y.ptr)
    assert name == "convtr"
    _check("convtr", y.f32().reshape(B, T * stride, Cout), ref, bound, f"convtr T{T} Cin{Cin} stride{stride}")


@pytest.mark.parametrize("R,C,s32", [(R, C, 0) for R in T_LIST for C in (5, 33, 512)] + [(R, C, 1) for R in (32, 256, 992) for C in (1, 7, 33, 512)])
def test_transpose(R, C, s32):
    """[B][R][C] -> [B][C][R]: fp32 copies are exact; S32 rows of R values are within the encoding's 22 bits."""
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(R + C)
    B = 2
    x = torch.randn(B, R, C, generator=gen).float()
    x[0, R - 1, C - 1] = 60000.0
    xd = _dev(x)
    y = Out(B * R * C)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    name, f = probe(_capi.WT_OP_TRANSPOSE, B=B, L=R, C=C, out_s32=s32, x=_p(xd), y=y.ptr, status=_p(status))
    assert name == "transpose" and (f.grid_x, f.grid_y, f.grid_z) == ((C + 31) // 32, (R + 31) // 32, B)
    want = x.transpose(1, 2).contiguous()
    if s32:
        got = G.decode_s32_rows(y.i16(), B * C, R).reshape(B, C, R)
        _check("transpose", got, want.double(), O.s32(want.double(), 0), f"transpose S32 R{R} C{C}")
    else:
        assert torch.equal(y.f32().reshape(B, C, R), want)
    assert int(status[0]) == 0


# ================================================================================================== reductions
@pytest.mark.parametrize("rows,D,fam", [(1, 512, "normal"), (5, 4, "normal"), (1000, 512, "spike"), (7, 516, "mean100"), (3, 256, "tiny"), (3, 1024, "huge")])
def test_row_sumsq(rows, D, fam):
    from wavtokenizer_amd import _capi
    x = family(fam, (rows, D), torch.Generator().manual_seed(rows + D)).float()
    ref, bound = O.row_sumsq(x.double())
    xd = _dev(x)
    y = Out(rows)
    name, f = probe(_capi.WT_OP_ROW_SUMSQ, n=rows, C=D, x=_p(xd), y=y.ptr)
    assert name == "row_sumsq" and f.grid_x == (rows + 3) // 4
    _check("row_sumsq", y.f32(), ref, bound, f"row_sumsq {rows}x{D} {fam}")


def _encode_s32(v):
    """fp32 values [n] (n % 32 == 0) -> the int16 halves of their S32 form."""
    hi = v.half()
    lo = ((v - hi.float()) * 2048.0).half()
    return torch.stack([hi.reshape(-1, 32), lo.reshape(-1, 32)], 1).reshape(-1).view(torch.int16)


@pytest.mark.parametrize("n,big", [(32, 3.5), (64 * 1000 + 32, -60000.0), (256 * 2048 * 2 + 96, 1234.56), (4096, 0.0)])
def test_s32_amax(n, big):
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(n)
    v = torch.randn(n, generator=gen).float() * 0.5
    if big:
        v[n - 7] = big
    else:
        v.zero_()
    h = _encode_s32(v)
    val = G.decode_s32_rows(h, n // 32, 32).abs().max().item()
    xd = h.cuda()
    y = Out(1, fill_nan=False)
    y.buf[GUARD] = 0
    name, _f = probe(_capi.WT_OP_S32_AMAX, n=n, x=xd.data_ptr(), y=y.ptr)
    assert name == "s32_amax"
    got = float(y.host().view(torch.float32)[0])
    assert abs(got - val) <= O.ULP * abs(val), (got, val)


# ======================================================================================= S32 range status
@pytest.mark.parametrize("op", ["gn_tile", "gn_chunk", "gn_stats", "rownorm", "dwconv_ln1", "dwconv_ln4", "transpose"])
@pytest.mark.parametrize("big,flag", [(65503.0, 0), (65504.0, 2)])
def test_s32_range_status(op, big, flag):
    """An S32 output whose largest value is just below 65504 leaves the status word clear; one at 65504 sets
    WT_STATUS_RANGE.  The value is placed exactly: a channel with gamma (out_scale) 0 and beta (out_shift) = big."""
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(3)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    if op.startswith("gn"):
        B, L, C = 2, {"gn_tile": 100, "gn_chunk": 300, "gn_stats": 300}[op], 768
        x, g, b = torch.randn(B, L, C, generator=gen), torch.ones(C), torch.zeros(C)
        g[C - 1], b[C - 1] = 0.0, big
        xd, gd, bd = _dev(x), _dev(g), _dev(b)
        y, sc, sh = Out(B * L * C), Out(B * C), Out(B * C)
        pt = torch.zeros(B * 32 * 3 * 2, device="cuda") if op != "gn_stats" else None
        name, _f = probe(_capi.WT_OP_GN_APPLY, B=B, L=L, C=C, groups=32, eps=1e-6, flag=0, out_s32=1, x=_p(xd), p0=_p(gd), p1=_p(bd),
                         p2=_p(pt), y=y.ptr, y2=sc.ptr, y3=sh.ptr, status=_p(status))
        assert name.startswith(op)
        got = G.decode_s32_rows(y.i16(), B * L, C)[:, C - 1]
    elif op == "transpose":
        x = torch.randn(1, 64, 40, generator=gen)
        x[0, 63, 39] = -big
        xd = _dev(x)
        y = Out(64 * 40)
        name, _f = probe(_capi.WT_OP_TRANSPOSE, B=1, L=64, C=40, out_s32=1, x=_p(xd), y=y.ptr, status=_p(status))
        got = G.decode_s32_rows(y.i16(), 40, 64)[39, 63:].abs()
    else:
        mode = 1 if op == "rownorm" else 0
        B, L, C = (700, 3, 512) if op == "dwconv_ln4" else (2, 9, 512)
        x, os_, oh = torch.randn(B, L, C, generator=gen), torch.ones(C), torch.zeros(C)
        os_[5], oh[5] = 0.0, big
        t = [_dev(v) for v in (x, torch.randn(7, C, generator=gen), torch.randn(C, generator=gen), os_, oh)]
        y = Out(B * L * C)
        name, _f = probe(_capi.WT_OP_ROWNORM, mode=mode, B=B, L=L, C=C, eps=1e-6, out_s32=1, x=_p(t[0]), p0=_p(t[1]), p1=_p(t[2]),
                         p4=_p(t[3]), p5=_p(t[4]), y=y.ptr, status=_p(status))
        assert name == {"rownorm": "rownorm<2,1>", "dwconv_ln1": "dwconv_ln<2,1>", "dwconv_ln4": "dwconv_ln<2,4>"}[op]
        got = G.decode_s32_rows(y.i16(), B * L, C)[:, 5]
    assert bool((got == big).all()), got[:4]
    assert int(status[0]) & 2 == flag, (op, big, int(status[0]))
    assert int(status[1]) == 0


# ============================================================================================ form coverage
# every (kernel, template value) the launchers of ops.hip can pick for these ops, read from launch_gn_apply, launch_gn_stats,
# launch_gn_chunked, launch_rownorm_nv, launch_softmax, launch_conv_last and the single-kernel launchers
ALL_FORMS = ({"gn_tile<0,1>", "gn_tile<0,2>", "gn_tile<1,1>", "gn_tile<1,2>", "gn_chunk<0>", "gn_chunk<1>", "gn_chunk<2>",
              "gn_stats<0>", "gn_stats<1>", "gn_stats<2>"}
             | {f"rownorm<{nv},{m}>" for nv in (1, 2, 3, 4) for m in (1, 2)}
             | {f"dwconv_ln<{nv},{r}>" for nv in (1, 2, 3, 4) for r in (1, 4)}
             | {f"softmax_reg<{n}>" for n in (1, 2, 5, 8)}
             | {"softmax_rmw", "istft_ola", "conv_first", "conv_last32", "conv_last", "transpose", "convtr", "row_sumsq", "s32_amax"})


def test_every_launch_form_was_reached():
    """Runs last: the forms the cases above reported are all the forms the launchers can pick; the worst fraction of the
    bound per op goes to the parity log (none above 1: the cases assert it)."""
    for op, w in sorted(WORST.items()):
        parity_log.record(f"op {op}", worst_of_bound=w)
        print(f"op {op}: worst error {w:.3g} of the bound")
    assert HIT == ALL_FORMS, (sorted(ALL_FORMS - HIT), sorted(HIT - ALL_FORMS))
