"""The length-aware launches of csrc/ops_kernel.inc (OPS_MIX 1: the kernels of a WT_PLAN_DECODE_MIXED plan), one launch at a time
through wt_op_probe with a lengths pointer.  Per family: a clip's valid rows are the bits of the same op probed alone at that
clip's length and pass the float64 bound of tests/op_ref.py, its pad rows are zeros whatever the input held there (NaN here),
the guard words around every output are intact, and the launch reports its form."""
import ctypes

import pytest
import torch

from tests import gemm_ref as G
from tests import op_ref as O

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -559038737                # 0xDEADBEEF


class Out:
    """A device output of n fp32 words between two guard runs, pre-filled with NaN (every logical element must be written)."""

    def __init__(self, n):
        self.n = n
        h = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32)
        h[GUARD:GUARD + n] = 0x7FC00000
        self.buf = h.cuda()
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def host(self):
        h = self.buf.cpu()
        assert bool((h[:GUARD] == SENT).all()) and bool((h[GUARD + self.n:] == SENT).all()), "guard words overwritten"
        return h[GUARD:GUARD + self.n]


def _dev(t):
    return None if t is None else t.float().contiguous().cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def probe(op, **kw):
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
    return _capi.WT_OPK_NAMES[f.kernel], f


def _lens(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device="cuda")


def _check(got, ref, bound, what):
    nbad, frac, finite = G.check(got, ref, bound)
    assert finite, f"{what}: an element was not written or is not finite"
    assert nbad == 0, f"{what}: {nbad} elements outside the bound (worst {frac:.3g} x bound)"


def _decode(row_bits, n_rows, C, s32):
    if s32:
        return G.decode_s32_rows(row_bits.contiguous().view(torch.int16).reshape(-1), n_rows, C).reshape(n_rows, C)
    return row_bits.contiguous().view(torch.float32).reshape(n_rows, C)


def test_old_descriptor_size_is_still_taken():
    """The lengths pointer is the struct's last field and optional: a caller built against the struct without it passes."""
    from wavtokenizer_amd import _capi
    x = torch.randn(2, 8, 4).cuda()
    y = Out(2 * 8 * 4)
    d = _capi.WtOpDesc()
    d.size = _capi.WtOpDesc.lengths.offset
    d.op, d.B, d.L, d.C, d.x, d.y = _capi.WT_OP_TRANSPOSE, 2, 8, 4, _p(x), y.ptr
    d.lengths = 0x10                                     # not read at this size
    f = _capi.WtOpForm()
    assert _capi.lib.wt_op_probe(ctypes.byref(d), ctypes.byref(f), None) == 0, _capi.lib.wt_last_error()
    torch.cuda.synchronize()
    assert _capi.WT_OPK_NAMES[f.kernel] == "transpose"
    assert torch.equal(y.host().view(torch.float32).reshape(2, 4, 8), x.cpu().transpose(1, 2))
    d.size += 4
    assert _capi.lib.wt_op_probe(ctypes.byref(d), ctypes.byref(f), None) == _capi.WT_ERR_INVALID


# ================================================================================================ GroupNorm
GN_LENGTHS = [1, 255, 256, 257, 385]       # C = 768: slab up to 256 frames, chunked above; 257 and 385: 3 and 4 chunks


def _gn(B, L, C, x, gamma, beta, swish, s32, apply, lengths=None):
    from wavtokenizer_amd import _capi
    xd, gd, bd = _dev(x), _dev(gamma), _dev(beta)
    y, sc, sh = Out(B * L * C), Out(B * C), Out(B * C)
    pt = torch.zeros(B * 32 * ((L + 127) // 128) * 2, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    lens = _lens(lengths) if lengths is not None else None
    kw = dict(B=B, L=L, C=C, groups=32, eps=1e-6, x=_p(xd), p0=_p(gd), p1=_p(bd), p2=_p(pt), y2=sc.ptr, y3=sh.ptr,
              status=_p(status), lengths=_p(lens))
    if apply:
        name, f = probe(_capi.WT_OP_GN_APPLY, flag=swish, out_s32=s32, y=y.ptr, **kw)
    else:
        name, f = probe(_capi.WT_OP_GN_STATS, **kw)
    assert int(status[0]) == 0
    return name, f, y.host(), sc.host(), sh.host()


@pytest.mark.parametrize("L_pad", [385, 416])
@pytest.mark.parametrize("swish,s32,apply", [(1, 1, True), (0, 0, True), (1, 0, True), (0, 0, False)])
def test_groupnorm(L_pad, swish, s32, apply):
    C, B = 768, len(GN_LENGTHS)
    gen = torch.Generator().manual_seed(L_pad + swish)
    x = torch.randn(B, L_pad, C, generator=gen) + 0.5
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    xin = x.clone()
    for b, Lb in enumerate(GN_LENGTHS):
        xin[b, Lb:] = float("nan")                       # rows past a clip's length are never read
    name, f, yb, sc, sh = _gn(B, L_pad, C, xin, gamma, beta, swish, s32, apply, GN_LENGTHS)
    assert name == "gn_mixed" and f.variant == ((2 if swish else 1) if apply else 0)
    assert f.variant2 == 3                               # both forms launched: L_pad is past both thresholds
    if apply:
        assert f.block == 512 and f.lds == 256 * 96 * 4 and (f.grid_x, f.grid_y) == (8, B)     # the slab sized by its limit
    for b, Lb in enumerate(GN_LENGTHS):
        xs = x[b:b + 1, :Lb].clone()
        sname, _f, ys, scs, shs = _gn(1, Lb, C, xs, gamma, beta, swish, s32, apply)
        want = ("gn_tile" if Lb <= 256 else "gn_chunk") if apply else ("gn_stats" if Lb <= 256 else "gn_chunk")
        assert sname == want
        assert torch.equal(sc.reshape(B, C)[b], scs) and torch.equal(sh.reshape(B, C)[b], shs), (b, Lb)
        ref = O.groupnorm(xs.double(), gamma.double(), beta.double(), 32, 1e-6, act=bool(swish), out_s32=bool(s32))
        _check(sc.view(torch.float32).reshape(B, C)[b:b + 1], *ref["scale"], f"scale L{Lb}")
        _check(sh.view(torch.float32).reshape(B, C)[b:b + 1], *ref["shift"], f"shift L{Lb}")
        if not apply:
            continue
        rows = yb.reshape(B, L_pad, C)[b]
        assert torch.equal(rows[:Lb].reshape(-1), ys), (b, Lb)
        assert bool((rows[Lb:] == 0).all()), (b, Lb)
        _check(_decode(rows[:Lb], Lb, C, s32).reshape(1, Lb, C), *ref["y"], f"y L{Lb}")


def test_groupnorm_slab_only():
    """A padded length within the slab limit: one launch, the slab sized by the padded length."""
    C, lengths, L_pad = 768, [1, 7, 120, 128], 128
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, L_pad, C, generator=gen)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    name, f, yb, _sc, _sh = _gn(4, L_pad, C, x, gamma, beta, 1, 1, True, lengths)
    assert name == "gn_mixed" and f.variant2 == 1 and f.lds == L_pad * 96 * 4
    for b, Lb in enumerate(lengths):
        _n, _f, ys, _a, _b = _gn(1, Lb, C, x[b:b + 1, :Lb].clone(), gamma, beta, 1, 1, True)
        rows = yb.reshape(4, L_pad, C)[b]
        assert torch.equal(rows[:Lb].reshape(-1), ys) and bool((rows[Lb:] == 0).all()), Lb


# ================================================================================================ dwconv + LayerNorm
def _dwconv(B, L, C, x, p, s32, lengths=None):
    from wavtokenizer_amd import _capi
    t = [_dev(v) for v in (x,) + p]
    y = Out(B * L * C)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    lens = _lens(lengths) if lengths is not None else None
    name, f = probe(_capi.WT_OP_ROWNORM, mode=0, B=B, L=L, C=C, eps=1e-6, out_s32=s32, x=_p(t[0]), p0=_p(t[1]), p1=_p(t[2]),
                    p4=_p(t[3]), p5=_p(t[4]), y=y.ptr, status=_p(status), lengths=_p(lens))
    assert int(status[0]) == 0
    return name, f, y.host()


@pytest.mark.parametrize("L_pad,lengths,R", [(703, [703, 701, 5, 2], 4), (704, [703, 698, 1, 3], 4), (100, [99, 100, 1, 6], 1)])
@pytest.mark.parametrize("s32", [0, 1])
def test_dwconv_ln(L_pad, lengths, R, s32):
    C, B = 768, len(lengths)
    gen = torch.Generator().manual_seed(L_pad + s32)
    x = torch.randn(B, L_pad, C, generator=gen)
    p = (torch.randn(7, C, generator=gen) / 7 ** 0.5, torch.randn(C, generator=gen), torch.randn(C, generator=gen) * 0.5 + 1,
         torch.randn(C, generator=gen))
    xin = x.clone()
    for b, Lb in enumerate(lengths):
        xin[b, Lb:] = float("nan")                       # taps at or past a clip's length are never read
    name, f, yb = _dwconv(B, L_pad, C, xin, p, s32, lengths)
    assert name == "dwconv_ln_mixed" and (f.variant, f.variant2) == (3, R) and (B * L_pad > 2048) == (R == 4)
    for b, Lb in enumerate(lengths):
        xs = x[b:b + 1, :Lb].clone()
        sname, _f, ys = _dwconv(1, Lb, C, xs, p, s32)
        assert sname == "dwconv_ln"
        rows = yb.reshape(B, L_pad, C)[b]
        assert torch.equal(rows[:Lb].reshape(-1), ys), (b, Lb)
        assert bool((rows[Lb:] == 0).all()), (b, Lb)
        ref, bound = O.rownorm(0, xs.double(), p[2].double(), p[3].double(), 1e-6, p[0].double(), p[1].double(), None, None, out_s32=bool(s32))
        _check(_decode(rows[:Lb], Lb, C, s32).reshape(1, Lb, C), ref, bound, f"dwconv L{Lb}")


# ==================================================================================================== softmax
def _softmax(rows, L, ld, s, s32, misalign=0, lengths=None):
    """s [rows][L] scores in a matrix of pitch ld whose pad columns hold NaN; returns (form, [rows][ld] fp32 words or S32 halves)."""
    from wavtokenizer_amd import _capi
    S = Out(rows * ld + 4)
    h = torch.full((rows, ld), float("nan"))
    h[:, :s.shape[1]] = s
    S.buf[GUARD + misalign:GUARD + misalign + rows * ld] = h.reshape(-1).view(torch.int32).cuda()
    if misalign:
        S.buf[GUARD] = SENT
    S.buf[GUARD + misalign + rows * ld:GUARD + rows * ld + 4] = SENT
    P = Out(rows * ld) if s32 else None
    lens = _lens(lengths) if lengths is not None else None
    name, f = probe(_capi.WT_OP_SOFTMAX, n=rows, L=L, ld=ld, x=S.ptr + 4 * misalign, y=P.ptr if s32 else None, lengths=_p(lens))
    sh = S.host()
    assert bool((sh[misalign + rows * ld:] == SENT).all()) and (not misalign or int(sh[0]) == SENT)
    if s32:      # per row and column the (hi, lo) pair
        return name, f, P.host().view(torch.int16).reshape(rows, -1, 2, 32).permute(0, 1, 3, 2).reshape(rows, ld, 2)
    return name, f, sh[misalign:misalign + rows * ld].reshape(rows, ld, 1)


# (L_pad, ld) as the pitches of SM_CASES (tests/test_decoder_ops.py): every register form and the read-modify-write kernel
@pytest.mark.parametrize("L_pad,ld,s32,mis", [(32, 32, 0, 0), (255, 256, 1, 0), (288, 288, 0, 0), (512, 512, 1, 0), (544, 544, 0, 0),
                                              (1249, 1280, 1, 0), (1312, 1312, 0, 0), (2080, 2080, 1, 0), (513, 544, 0, 1)])
def test_softmax(L_pad, ld, s32, mis):
    lengths = sorted({1, 2, min(33, L_pad), L_pad // 2 + 1, L_pad - 1, L_pad})
    B = len(lengths)
    nq = 3                                               # query rows checked per clip: the first, one inside, the last
    gen = torch.Generator().manual_seed(L_pad + ld)
    s = torch.randn(B, L_pad, L_pad, generator=gen) * 3
    name, f, got = _softmax(B * L_pad, L_pad, ld, s.reshape(B * L_pad, L_pad), s32, mis, lengths)
    nv = 1 if ld <= 256 else 2 if ld <= 512 else 5 if ld <= 1280 else 8
    assert (name, f.variant) == (("softmax_rmw_mixed", 0) if (mis or ld > 2048) else ("softmax_reg_mixed", nv))
    assert f.grid_x == (B * L_pad + 3) // 4
    got = got.reshape(B, L_pad, ld, -1)
    for b, Lb in enumerate(lengths):
        q = sorted({0, Lb // 2, L_pad - 1})[:nq]
        ss = s[b, q, :Lb].contiguous()
        ldb = (Lb + 31) // 32 * 32                       # the pitch of a call of the clip's own length
        _n, _f, solo = _softmax(len(q), Lb, ldb, ss, s32)
        assert torch.equal(got[b, q, :Lb], solo[:, :Lb]), (b, Lb)
        assert bool((got[b, :, Lb:] == 0).all()), (b, Lb)
        ref, bound = O.softmax(ss.double(), out_s32=bool(s32))
        words = got[b, q, :Lb]
        val = (words[..., 0].contiguous().view(torch.float16).double() + words[..., 1].contiguous().view(torch.float16).double() / 2048) \
            if s32 else words[..., 0].contiguous().view(torch.float32).double()
        _check(val, ref, bound, f"softmax L{Lb}")


# ================================================================================================== ISTFT tail
@pytest.mark.parametrize("n_fft,hop", [(2400, 600), (1280, 320)])
@pytest.mark.parametrize("center", [0, 1])
def test_istft_ola(n_fft, hop, center):
    from wavtokenizer_amd import _capi
    L_pad, lengths = 6, [1, 2, 3, 6]
    B = len(lengths)
    Kq = (n_fft // 4 + 1 + 31) // 32 * 32
    gen = torch.Generator().manual_seed(n_fft + center)
    parts = torch.randn(4, B, L_pad, Kq, generator=gen).float()
    pin = parts.clone()
    for b, Lb in enumerate(lengths):
        pin[:, b, Lb:] = float("nan")                    # frames at or past a clip's length are never read
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64).float()
    wd, qd = _dev(win), _dev(win * win)
    T = hop * (L_pad - 1 if center else L_pad)
    y = Out(B * T)
    pd, lens = _dev(pin), _lens(lengths)
    name, f = probe(_capi.WT_OP_ISTFT_OLA, B=B, L=L_pad, n_fft=n_fft, hop=hop, Kq=Kq, flag=center, x=_p(pd), p0=_p(wd), p1=_p(qd),
                    y=y.ptr, lengths=_p(lens))
    assert name == "istft_ola_mixed" and f.grid_x == (-(-(B * T) // 256) + 7) // 8 * 8
    got = y.host().reshape(B, T)
    for b, Lb in enumerate(lengths):
        Tb = hop * (Lb - 1 if center else Lb)
        assert bool((got[b, Tb:] == 0).all()), (b, Lb)
        if Tb == 0:
            continue
        ps = parts[:, b:b + 1, :Lb].contiguous()
        ys = Out(Tb)
        psd = _dev(ps)
        sname, _f = probe(_capi.WT_OP_ISTFT_OLA, B=1, L=Lb, n_fft=n_fft, hop=hop, Kq=Kq, flag=center, x=_p(psd), p0=_p(wd), p1=_p(qd), y=ys.ptr)
        assert sname == "istft_ola"
        assert torch.equal(got[b, :Tb], ys.host()), (b, Lb)
        ref, bound = O.istft_tail(ps.double(), win.double(), n_fft, hop, bool(center))
        _check(got[b:b + 1, :Tb].contiguous().view(torch.float32), ref, bound, f"istft L{Lb}")


# =================================================================================================== transpose
@pytest.mark.parametrize("s32", [0, 1])
def test_transpose(s32):
    """[B][R channels][C frames] -> [B][C][R]: frames at or past a clip's length become zero rows, whatever they held."""
    from wavtokenizer_amd import _capi
    R, C, lengths = 512, 70, [1, 31, 32, 33, 70]
    B = len(lengths)
    gen = torch.Generator().manual_seed(s32)
    x = torch.randn(B, R, C, generator=gen).float()
    xin = x.clone()
    for b, Lb in enumerate(lengths):
        xin[b, :, Lb:] = float("nan")
    xd, lens = _dev(xin), _lens(lengths)
    y = Out(B * C * R)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    name, f = probe(_capi.WT_OP_TRANSPOSE, B=B, L=R, C=C, out_s32=s32, x=_p(xd), y=y.ptr, status=_p(status), lengths=_p(lens))
    assert name == "transpose_mixed" and (f.grid_x, f.grid_y, f.grid_z) == ((C + 31) // 32, R // 32, B)
    assert int(status[0]) == 0
    got = y.host().reshape(B, C, R)
    for b, Lb in enumerate(lengths):
        xs = _dev(x[b:b + 1, :, :Lb])
        ys = Out(Lb * R)
        sname, _f = probe(_capi.WT_OP_TRANSPOSE, B=1, L=R, C=Lb, out_s32=s32, x=_p(xs), y=ys.ptr)
        assert sname == "transpose"
        assert torch.equal(got[b, :Lb].reshape(-1), ys.host()), (b, Lb)
        assert bool((got[b, Lb:] == 0).all()), (b, Lb)
        if not s32:
            assert torch.equal(got[b, :Lb].contiguous().view(torch.float32), x[b, :, :Lb].t())
