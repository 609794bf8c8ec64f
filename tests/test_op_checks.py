"""CPU-only halves of tests/test_decoder_ops.py: for every op the bounds of tests/op_ref.py pass an honest fp32 evaluation
(torch fp32, the same formula, two summation orders) on every input family with 0 bad elements, the checker rejects each
slip it exists for (the docstrings say on which family), and wt_op_probe refuses bad descriptors before any HIP call (so
these run on a host without a GPU)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as G
from tests import op_ref as O

FAMILIES = ["normal", "mean100", "const", "spike", "tiny", "huge", "small"]
f32, f64 = torch.float32, torch.float64


def family(name, shape, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=gen)
    if name == "mean100":
        x = x + 100.0
    elif name == "const":
        x = torch.full(shape, 3.0)
    elif name == "spike":
        x = x * 1e-3
        x.reshape(-1)[:: max(1, x.numel() // 7) + 1] = 1e4
    elif name == "tiny":
        x = x * 1e-20
    elif name == "huge":
        x = x * 1e15
    elif name == "small":                # variance about eps = 1e-6
        x = x * 1e-3
    elif name == "wide":
        x = torch.rand(*shape, generator=gen) * 200 - 100
    return x.float()


def ok(got, ref, bound):
    bad, worst, finite = G.check(got, ref, bound)
    return finite and bad == 0, worst


def rejected(got, wrong_ref, bound):
    bad, _w, finite = G.check(got, wrong_ref, bound)
    return bad > 0 or not torch.isfinite(wrong_ref).all()


# ================================================================================================ GroupNorm
def gsum(t):
    """Sum of t [B][rows][groups][cg] per (clip, group) over a contiguous run: torch's cascaded sum, whose depth stays
    within the one op_ref.sum_k assumes (a reduction over the strided axes adds each column serially: depth `rows`)."""
    B, _r, g, _c = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, g, -1).sum(-1).reshape(B, 1, g, 1)


def gn_eval(x, gamma, beta, groups, eps, dtype, order=0, act=False, slip=None):
    """GroupNorm in `dtype` as scale / shift; order 0: one sum per group, order 1: 128-row chunks merged with Chan's update
    (the chunked kernels' scheme).  slip: one deliberate mistake."""
    B, L, C = x.shape
    cg = C // groups
    xg = x.to(dtype).reshape(B, L, groups, cg)
    g, b = gamma.to(dtype).reshape(1, 1, groups, cg), beta.to(dtype).reshape(1, 1, groups, cg)
    if slip == "neighbour_group":
        g, b = g.roll(1, 2), b.roll(1, 2)
    xs = xg[:, :L - 1] if (slip == "one_row_short" and L > 1) else xg
    n = xs.shape[1] * cg
    if order == 0 and slip != "no_between_term":
        mean = gsum(xs) / n
        m2 = gsum((xs - mean) ** 2)
    else:
        cnt, mean, m2 = 0, torch.zeros(B, 1, groups, 1, dtype=dtype), torch.zeros(B, 1, groups, 1, dtype=dtype)
        for t0 in range(0, xs.shape[1], 128):
            ch = xs[:, t0:t0 + 128]
            nq = ch.shape[1] * cg
            mq = gsum(ch) / nq
            sq = gsum((ch - mq) ** 2)
            d, tot = mq - mean, cnt + nq
            mean = mean + d * (nq / tot)
            m2 = m2 + sq + (0 if slip == "no_between_term" else d * d * (cnt * nq / tot))
            cnt = tot
    var = m2 / (n - 1 if slip == "unbiased" else n)
    if slip == "no_eps":
        rstd = 1.0 / torch.sqrt(var)
    elif slip == "eps_outside":
        rstd = 1.0 / (torch.sqrt(var) + eps)
    else:
        rstd = 1.0 / torch.sqrt(var + eps)
    sc = rstd * g
    sh = b - mean * sc
    y = xg * sc + sh
    if act:
        y = y * torch.sigmoid(y)
    return y.reshape(B, L, C).double(), sc.expand(B, 1, groups, cg).reshape(B, C).double(), sh.expand(B, 1, groups, cg).reshape(B, C).double()


@pytest.mark.parametrize("fam", FAMILIES + ["swishwide"])
@pytest.mark.parametrize("L,C", [(1, 768), (7, 768), (256, 768), (385, 768), (130, 96), (300, 512)])
def test_groupnorm_bound_passes_honest_fp32(fam, L, C):
    x = family("normal" if fam == "swishwide" else fam, (2, L, C), seed=L)
    gen = torch.Generator().manual_seed(1)
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).float(), torch.randn(C, generator=gen).float()
    if fam == "swishwide":
        beta = torch.linspace(-100, 100, C).float()
    for act in (False, True):
        ref = O.groupnorm(x.double(), gamma.double(), beta.double(), 32, 1e-6, act=act)
        for order in (0, 1):
            y, sc, sh = gn_eval(x, gamma, beta, 32, 1e-6, f32, order, act)
            for got, key in ((y, "y"), (sc, "scale"), (sh, "shift")):
                good, worst = ok(got, *ref[key])
                assert good, (fam, L, C, act, order, key, worst)


GN_SLIPS = {                       # slip -> (family, L) on which it must be rejected
    "unbiased": ("normal", 7), "no_eps": ("const", 130), "eps_outside": ("small", 130), "one_row_short": ("normal", 129),
    "no_between_term": ("mean100", 385), "neighbour_group": ("normal", 130),
}


@pytest.mark.parametrize("slip", sorted(GN_SLIPS))
def test_groupnorm_checker_rejects(slip):
    """unbiased variance: unit normal, L = 7 (n = 168); eps omitted: the constant family (rstd = inf); eps outside the
    root: unit normal x 1e-3, whose variance is about eps (at magnitudes 1e-20 the difference drowns in beta); statistics one row short (the chunk-tail bug): unit normal at
    L = 129; chunk merge without d^2 n nq / tot: the mean-100 family at L = 385 with a ramp of 0.01 per frame added, so
    that the chunk means differ;
    gamma / beta of the neighbouring group: unit normal."""
    fam, L = GN_SLIPS[slip]
    C = 768
    x = family(fam, (2, L, C), seed=3)
    if slip == "no_between_term":
        x = x + torch.arange(L).float()[None, :, None] * 0.01
    gen = torch.Generator().manual_seed(1)
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).float(), torch.randn(C, generator=gen).float()
    ref = O.groupnorm(x.double(), gamma.double(), beta.double(), 32, 1e-6)
    got, _sc, _sh = gn_eval(x, gamma, beta, 32, 1e-6, f32)
    assert ok(got, *ref["y"])[0]
    wrong, _sc, _sh = gn_eval(x, gamma, beta, 32, 1e-6, f64, slip=slip)
    assert rejected(got, wrong, ref["y"][1]), slip


# ================================================================================================== row norms
def rn_eval(mode, x, os_, oh, eps, dtype, order=0, dw_w=None, dw_b=None, isc=None, ish=None, slip=None):
    B, L, C = x.shape
    x = x.to(dtype)
    if mode == 0:
        w = dw_w.to(dtype)
        if slip == "taps_reversed":
            w = w.flip(0)
        if slip == "wrap":                       # the clips treated as one sequence: taps reach into the neighbouring clip
            xp = F.pad(x.reshape(1, B * L, C), (0, 0, 3, 3)).expand(1, -1, -1)
            v = dw_b.to(dtype).expand(1, B * L, C).clone()
            for j in range(7):
                v = v + xp[:, j:j + B * L] * w[j]
            v = v.reshape(B, L, C)
        else:
            xp = F.pad(x, (0, 0, 3, 3))
            v = dw_b.to(dtype).expand(B, L, C).clone()
            for j in (range(7) if order == 0 else range(6, -1, -1)):
                v = v + xp[:, j:j + L] * w[j]
    elif mode == 2:
        v = x * isc.to(dtype)[:, None] + ish.to(dtype)[:, None]
    else:
        v = x
    if order == 0:
        mean = v.mean(-1, keepdim=True)
        var = ((v - mean) ** 2).mean(-1, keepdim=True)
    else:
        mean = v.reshape(B, L, 4, C // 4).sum(-1).sum(-1, keepdim=True) / C
        var = ((v - mean) ** 2).reshape(B, L, 4, C // 4).sum(-1).sum(-1, keepdim=True) / C
    if slip == "unbiased":
        var = var * C / (C - 1)
    rstd = 1.0 / torch.sqrt(var + (0 if slip == "no_eps" else eps))
    return (((v - mean) * rstd) * os_.to(dtype) + oh.to(dtype)).double()


def _rn_operands(C, B, seed=2):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen).float()
    return dict(os_=r(C) * 0.5 + 1, oh=r(C), dw_w=r(7, C) / 7 ** 0.5, dw_b=r(C), isc=torch.rand(B, C, generator=gen).float() + 0.5, ish=r(B, C))


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C,L", [(256, 5), (768, 50), (1024, 3)])
def test_rownorm_bound_passes_honest_fp32(mode, fam, C, L):
    B = 3
    x = family(fam, (B, L, C), seed=C + L)
    p = _rn_operands(C, B)
    d = {k: v.double() for k, v in p.items()}
    ref, bound = O.rownorm(mode, x.double(), d["os_"], d["oh"], 1e-6, d["dw_w"], d["dw_b"], d["isc"], d["ish"])
    for order in (0, 1):
        got = rn_eval(mode, x, p["os_"], p["oh"], 1e-6, f32, order, p["dw_w"], p["dw_b"], p["isc"], p["ish"])
        good, worst = ok(got, ref, bound)
        assert good, (mode, fam, C, L, order, worst)


@pytest.mark.parametrize("slip,mode,fam", [("taps_reversed", 0, "normal"), ("wrap", 0, "normal"), ("unbiased", 1, "normal"),
                                           ("no_eps", 1, "const"), ("other_bandwidth_row", 0, "normal")])
def test_rownorm_checker_rejects(slip, mode, fam):
    """dwconv taps reversed, taps wrapping into the neighbouring clip instead of zero padding, the AdaLayerNorm row of
    another bandwidth_id (another scale / shift vector), unbiased variance: unit normal, B = 3; eps omitted: constant rows."""
    B, L, C = 3, 9, 768
    x = family(fam, (B, L, C), seed=5)
    p = _rn_operands(C, B)
    d = {k: v.double() for k, v in p.items()}
    ref, bound = O.rownorm(mode, x.double(), d["os_"], d["oh"], 1e-6, d["dw_w"], d["dw_b"], d["isc"], d["ish"])
    got = rn_eval(mode, x, p["os_"], p["oh"], 1e-6, f32, 0, p["dw_w"], p["dw_b"], p["isc"], p["ish"])
    assert ok(got, ref, bound)[0]
    if slip == "other_bandwidth_row":
        q = _rn_operands(C, B, seed=77)
        wrong = rn_eval(mode, x, q["os_"], q["oh"], 1e-6, f64, 0, p["dw_w"], p["dw_b"])
    else:
        wrong = rn_eval(mode, x, p["os_"], p["oh"], 1e-6, f64, 0, p["dw_w"], p["dw_b"], p["isc"], p["ish"], slip=slip)
    assert rejected(got, wrong, bound), slip


# ==================================================================================================== softmax
def _scores(rows, L, seed=0):
    gen = torch.Generator().manual_seed(seed)
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


@pytest.mark.parametrize("L", [1, 2, 31, 257, 1200, 2079])
def test_softmax_bound_passes_honest_fp32(L):
    """Rows of every family (spreads 0, 1 and 200, the maximum in column 0 and in column L - 1) in one matrix."""
    s = _scores(14, L, seed=L)
    ref, bound = O.softmax(s.double())
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    for got in (torch.softmax(s, -1), e / e.flip(-1).sum(-1, keepdim=True), e / e.reshape(14, -1).cumsum(-1)[:, -1:]):
        good, worst = ok(got.double(), ref, bound)
        assert good, (L, worst)
        assert (got.double().sum(-1) - 1).abs().max() <= L * O.ULP


@pytest.mark.parametrize("slip", ["pad_in_sum", "neighbour_sum"])
def test_softmax_checker_rejects(slip):
    """Pad columns (zero scores) counted in the sum; a row divided by the neighbouring row's sum: rejected on the unit
    normal rows (and every other family of the matrix)."""
    s = _scores(14, 100)
    ref, bound = O.softmax(s.double())
    got = torch.softmax(s, -1).double()
    assert ok(got, ref, bound)[0]
    e = torch.exp(s.double() - s.double().max(-1, keepdim=True).values)
    if slip == "pad_in_sum":
        wrong = e / (e.sum(-1, keepdim=True) + 28 * torch.exp(-s.double().max(-1, keepdim=True).values))
    else:
        wrong = e / e.sum(-1, keepdim=True).roll(1, 0)
    assert rejected(got, wrong, bound)


# ================================================================================================== ISTFT tail
def _istft_operands(n_fft, B, L, seed=0):
    Kq = (n_fft // 4 + 1 + 31) // 32 * 32
    parts = torch.randn(4, B, L, Kq, generator=torch.Generator().manual_seed(seed)).float()
    win = torch.hann_window(n_fft, periodic=True, dtype=f64).float()
    return parts, win


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("n_fft,hop", [(2400, 600), (1280, 320)])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 40])
def test_istft_bound_passes_honest_fp32(n_fft, hop, L, center):
    if center and L == 1:
        return                                  # no output samples
    parts, win = _istft_operands(n_fft, 2, L, seed=L)
    ref, bound = O.istft_tail(parts.double(), win.double(), n_fft, hop, center)
    for reverse in (False, True):
        got, _b = O.istft_tail(parts, win, n_fft, hop, center, dtype=f32, reverse=reverse)
        good, worst = ok(got.double(), ref, bound)
        assert good, (n_fft, L, center, reverse, worst)


@pytest.mark.parametrize("slip", ["interior_envelope", "se_so_swapped", "trim_off_by_one"])
def test_istft_checker_rejects(slip):
    """The interior envelope used at the edges (the first and last n_fft / hop - 1 frames have fewer overlapping windows);
    Se and So exchanged (the sign of S[N/2 - m] = So - Se); the trim one sample off: unit normal parts, L = 6, 'same'."""
    n_fft, hop, L = 1280, 320, 6
    parts, win = _istft_operands(n_fft, 2, L)
    ref, bound = O.istft_tail(parts.double(), win.double(), n_fft, hop, False)
    got, _b = O.istft_tail(parts, win, n_fft, hop, False, dtype=f32)
    assert ok(got.double(), ref, bound)[0]
    if slip == "interior_envelope":
        mid, _b = O.istft_tail(parts.double()[:, :, :], win.double(), n_fft, hop, False)
        env_in = sum((win.double() ** 2)[r::hop].sum() for r in range(1)) * 0 + torch.stack([(win.double() ** 2)[r::hop].sum() for r in range(hop)])
        pad = (n_fft - hop) // 2
        T = hop * L
        u = torch.arange(T) + pad
        env_true = torch.zeros((L - 1) * hop + n_fft, dtype=f64)
        for t in range(L):
            env_true[t * hop:t * hop + n_fft] += win.double() ** 2
        wrong = ref * env_true[pad:pad + T] / env_in[u % hop]
    elif slip == "se_so_swapped":
        wrong, _b = O.istft_tail(parts.double()[[0, 1, 3, 2]], win.double(), n_fft, hop, False)
    else:
        wrong = torch.roll(ref, 1, -1)
    assert rejected(got.double(), wrong, bound)


# ================================================================================================= small convs
def test_reflect_padding_matches_the_oracle():
    """The index arithmetic of op_ref's reflect padding against the oracle's restatement of the reference's pad1d
    (short inputs included): a cross-check, not the reference."""
    from oracle.cpu_ref import pad1d_reflect
    for T in (1, 2, 3, 4, 9):
        x = torch.randn(2, 3, T, dtype=f64)
        assert torch.equal(O._reflect_pad_time(x, 3, 3), pad1d_reflect(x, (3, 3)))


@pytest.mark.parametrize("T", [1, 2, 3, 4, 257])
def test_conv_bounds_pass_honest_fp32(T):
    gen = torch.Generator().manual_seed(T)
    r = lambda *s: torch.randn(*s, generator=gen).float()
    wav, w, b = r(2, T), r(7, 32) / 7 ** 0.5, r(32)
    ref, bound = O.conv_first(wav.double(), w.double(), b.double())
    xp = O._reflect_pad_time(wav[:, None], 3, 3)[:, 0]
    for order in (range(7), range(6, -1, -1)):
        got = b.expand(2, T, 32).clone()
        for j in order:
            got = got + xp[:, j:j + T, None] * w[j]
        assert ok(got.double(), ref, bound)[0]
    for fam, elu_in in (("normal", False), ("normal", True), ("wide", True)):
        x, wl, bl = family(fam, (2, T, 32), seed=T), r(7, 32) / 15, r(1)
        ref, bound = O.conv_last(x.double(), wl.double(), bl.double(), elu_in)
        a = F.elu(x) if elu_in else x
        xp = O._reflect_pad_time(a.transpose(1, 2), 3, 3)
        got1 = F.conv1d(xp, wl.t()[None], bl)[:, 0]
        got2 = bl + sum((xp[:, :, j:j + T] * wl[j][None, :, None]).flip(1).sum(1) for j in range(6, -1, -1))
        for got in (got1, got2):
            good, worst = ok(got.double(), ref, bound)
            assert good, (fam, elu_in, worst)
        xt, wt, bt = family(fam, (2, T, 16), seed=T + 1), r(8, 16, 8) / 6, r(8)
        ref, bound = O.convtr(xt.double(), wt.double(), bt.double(), 4, elu_in)
        a = (F.elu(xt) if elu_in else xt).transpose(1, 2)
        full = F.conv_transpose1d(a, wt.permute(1, 2, 0), bt, stride=4)
        full2 = F.conv_transpose1d(a.flip(1), wt.permute(1, 2, 0).flip(0), bt, stride=4)
        for got in (full, full2):
            good, worst = ok(got[..., 2:full.shape[-1] - 2].transpose(1, 2).double(), ref, bound)
            assert good, (fam, elu_in, worst)
    x = family("spike", (5, 516), seed=T)
    ref, bound = O.row_sumsq(x.double())
    for got in ((x * x).sum(-1), (x * x).flip(-1).reshape(5, 4, -1).sum(-1).sum(-1)):
        assert ok(got.double(), ref, bound)[0]


def test_conv_checker_rejects_zero_padding_and_a_dropped_transpose_row():
    """Zero instead of reflect padding (conv_first and conv_last, unit normal, T = 50: the first and last 3 samples);
    a transpose that drops the last row of a partial 32 x 32 tile (R = 40: row 39), against the S32 encoding bound."""
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen).float()
    wav, w, b = r(2, 50), r(7, 32), r(32)
    ref, bound = O.conv_first(wav.double(), w.double(), b.double())
    zero = F.conv1d(F.pad(wav.double()[:, None], (3, 3)), w.double().t()[:, None], b.double()).transpose(1, 2)
    assert rejected(ref.float().double(), zero, bound)
    x, wl, bl = r(2, 50, 32), r(7, 32), r(1)
    ref, bound = O.conv_last(x.double(), wl.double(), bl.double(), False)
    zero = F.conv1d(F.pad(x.double().transpose(1, 2), (3, 3)), wl.double().t()[None], bl.double())[:, 0]
    assert rejected(ref.float().double(), zero, bound)
    t = r(2, 40, 33)
    want = t.transpose(1, 2).double()
    dropped = want.clone()
    dropped[:, :, 39] = 0
    assert ok(want, want, O.s32(want, 0))[0] and rejected(want, dropped, O.s32(want, 0))


# =================================================================================================== refusals
FAKE = 1 << 20          # aligned stand-ins for device pointers: a refused descriptor never dereferences them


def _desc(op, **kw):
    from wavtokenizer_amd import _capi
    d = _capi.WtOpDesc()
    d.size = ctypes.sizeof(d)
    d.op = op
    d.B, d.L, d.C, d.groups, d.eps = 2, 16, 768, 32, 1e-6
    d.n, d.ld, d.k, d.stride, d.Cout, d.n_fft, d.hop, d.Kq = 8, 32, 7, 2, 32, 1280, 320, 352
    for i, f in enumerate(("x", "p0", "p1", "p2", "p3", "p4", "p5", "y", "y2", "y3")):
        setattr(d, f, (i + 1) * FAKE)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("what,op,kw,msg", [
    ("rownorm C", 2, dict(C=384), "256, 512, 768 or 1024"),
    ("gn S32 with C % 32", 0, dict(C=80, groups=4, out_s32=1), "C % 32 == 0"),
    ("softmax S32 pitch", 3, dict(L=30, ld=40), "multiples of 32"),
    ("transpose S32 rows", 7, dict(L=40, out_s32=1), "multiples of 32"),
    ("conv_last Cin", 6, dict(C=24), "power of two"),
    ("conv_last Cin too wide", 6, dict(C=512), "power of two"),
    ("null pointer", 0, dict(p1=None), "null"),
    ("null x", 9, dict(x=None), "x missing"),
    ("misaligned", 2, dict(p4=6 * FAKE + 4), "16-byte"),
    ("wrong size", 0, dict(size=8), "another size"),
    ("unknown op", 11, dict(), "unknown op"),
    ("negative op", -1, dict(), "unknown op"),
    ("zero extent", 2, dict(L=0), "positive"),
    ("negative extent", 0, dict(B=-1), "positive"),
    ("softmax L > ld", 3, dict(L=33), "L <= ld"),
    ("groups", 0, dict(groups=7), "groups"),
    ("istft", 4, dict(hop=300), "n_fft % hop"),
    ("convtr", 8, dict(Cout=30), "Cout % 4"),
    ("s32_amax", 10, dict(n=40), "groups of 32"),
])
def test_op_probe_refuses_before_any_hip_call(what, op, kw, msg):
    """What the launchers refuse (and what they leave to the plans to get right) comes back as WT_ERR_INVALID with a
    message, before any HIP call: the pointers here are not even valid."""
    from wavtokenizer_amd import _capi
    d = _desc(op, **kw)
    assert _capi.lib.wt_op_probe(ctypes.byref(d), None, None) == -1, what
    assert msg in _capi.lib.wt_last_error().decode(), (what, _capi.lib.wt_last_error())
