"""gemm16h_kernel, the one-product twin of gemm16s_kernel (WT_PLAN_FLAG_F16_GEMM), alone: through wt_gemm_probe with engine = 2
on the case table of tests/test_gemm_epilogues.py, for the eight (epilogue, output format) pairs the decode plans use.
  1. every case runs on the tile form engine 0 reports for the same descriptor;
  2. on f16-exact operands (every lo half zero) engine 2 returns the bits of engine 0, the untouched padding included;
  3. on general operands every element lies within gemm_ref.epilogue's bound around the float64 product of the hi halves
     (tests/f16_ref.py: activations f16(v), weights f16(w s) / s): products of two f16 numbers are exact in fp32, so the
     accumulation term TOL of the three-product kernel covers this one with its margin;
  4. the mode is in effect: on operands with non-zero lo halves engine 2 is at least 10 x further from the float64 product of
     the unrounded operands than engine 0 (about 2^10 from the formats);
  5. what the twin does not exist for is refused before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

from tests import f16_ref
from tests import gemm_ref as G
from tests.test_gemm_checks import FAKE, _desc
from tests.test_gemm_epilogues import EXPECT16, EXPECT16_HEAD, _cases16, _form_name, _ncu, _ptr, _r, lin

# build_decode and plan_head on S32 operands (gemm16s.hip WT_GEMM16H_PAIRS)
PAIRS16H = [(G.EPI_BIAS, G.OUT_F32), (G.EPI_BIAS_RES, G.OUT_F32), (G.EPI_BIAS, G.OUT_S32), (G.EPI_BIAS_ROW, G.OUT_S32),
            (G.EPI_SCALE, G.OUT_F32), (G.EPI_BIAS_GELU, G.OUT_S32), (G.EPI_BIAS_GAMMA_RES, G.OUT_F32), (G.EPI_HEAD, G.OUT_S32)]
_ids = lambda p: f"{G.EPI_NAMES[p[0]]}-{G.OUT_NAMES[p[1]]}"
ALPHA = 0.0883883


def _problem(epi, c, seed, mode):
    """Operands of case c as fp32 tensors, in the layouts of test_gemm_epilogues._run.  mode "f16": random f16 values widened
    to fp32, the weight's maximum inside [2^-6, 2^12) (scale 1; the case's own weight scaling is left out); "general": fp32
    values as that test draws them; "unit": uniform in [1, 2)."""
    gen = torch.Generator().manual_seed(seed)
    if mode == "unit":
        rnd = lambda *s: torch.rand(*s, generator=gen) + 1.0
    else:
        rnd = lambda *s: torch.randn(*s, generator=gen)
    q = (lambda t: t.half().float()) if mode == "f16" else (lambda t: t.float())
    head = epi == G.EPI_HEAD
    nz, M, N, K = c.nz or 1, c.M, c.N, c.K
    wscale = 1.0 if mode == "f16" else (c.wscale or 1.0)
    P = dict(nz=nz, M=M, N=N, K=K, c=c, fields={})
    f = P["fields"]
    if c.kind == "conv":
        x = q(rnd(c.clips, c.Cin, c.T_in) / wscale)
        w = q(rnd(N, c.Cin, c.k) / (c.Cin * c.k) ** 0.5 * wscale)
        P["x"], P["w"] = x, w
        P["A"] = x.transpose(1, 2).contiguous().reshape(-1)
        order = G.tap_order(c.k, c.stride, c.tap_pair)
        P["Bw"] = w[:, :, order].permute(0, 2, 1).reshape(N, K).contiguous().reshape(-1)
        f.update(T_in=c.T_in, T_out=c.T_out, Cin=c.Cin, taps=c.k, stride=c.stride, dil=c.dil, pad_left=c.pl, pad_mode=c.pad_mode,
                 tap_pair=1 if c.tap_pair else 0, Tp=max(c.T_in, max(c.pl, c.pr) + 1) if c.pad_mode == 1 else c.T_in,
                 a_bstride=c.T_in * c.Cin, a_rstride=c.Cin, w_rstride=K)
        P["A2"] = None
    else:
        K1 = c.K1 or K
        arow = K1 + (c.apad or 0)
        na = 1 if c.shared else nz
        a_nat = q(rnd(na, M, K) / wscale)
        if head:
            kb = N // 2
            lm = rnd(nz, kb, K) / K ** 0.5 * wscale
            ph = rnd(nz, kb, K) / K ** 0.5 * 2 * wscale
            b_nat = q(torch.stack([G.pack_head_rows(lm[z], ph[z]) for z in range(nz)]))
        else:
            b_nat = q(rnd(nz, N, K) / K ** 0.5 * wscale)
        P["a_nat"], P["b_nat"], P["na"] = a_nat, b_nat, na
        Abuf = torch.zeros(na, M, arow)
        Abuf[:, :, :K1] = a_nat[:, :, :K1]
        P["A"] = Abuf.reshape(-1)
        P["A2"] = None
        if c.K1:
            P["A2"] = a_nat[0, :, K1:].contiguous().reshape(-1)
            f.update(K1=K1, a2_rstride=K - K1)
        P["Bw"] = b_nat.reshape(-1).contiguous()
        f.update(T_in=M, T_out=M, Cin=K, a_rstride=arow, w_rstride=K, zA=0 if c.shared else M * arow, zW=N * K)
    if mode == "f16" and not c.b_act:
        amax = float(P["Bw"].abs().max())
        assert 2.0 ** -6 <= amax < 2.0 ** 12, amax                 # s32_weight_scale is 1: the weight's lo halves are zero
    bias = R = gamma = None
    if epi == G.EPI_BIAS_ROW:
        bias = rnd(M).float()
    elif head:
        bias = torch.stack([G.pack_head_rows(torch.randn(N // 2, generator=gen) * 2 + 2, torch.randn(N // 2, generator=gen))]).reshape(-1).float()
    elif epi != G.EPI_SCALE and not c.no_bias:
        bias = rnd(N).float()
    r_pitch = _r(N, 4) + 32
    if epi in (G.EPI_BIAS_RES, G.EPI_BIAS_GAMMA_RES):
        R = rnd(M, r_pitch).float()
        f["r_rstride"] = r_pitch
    if epi == G.EPI_BIAS_GAMMA_RES:
        gamma = (torch.rand(N, generator=gen) + 0.25).float()
    if head:
        f["head_kb"] = N // 2
    P.update(bias=bias, R=R, gamma=gamma)
    return P


def _products(P, a_of, w_of):
    """(acc, mag) [nz][M][N] in float64 of the problem's contraction, its activations seen through a_of and its B operand
    through w_of (identity: the unrounded operands; f16_ref.act_hi / weight_hi: what the twin multiplies)."""
    c, nz, M, N = P["c"], P["nz"], P["M"], P["N"]
    if c.kind == "conv":
        acc, mag = G.conv_ref(a_of(P["x"]), w_of(P["w"]), c.stride, c.dil, c.pl, c.pr, c.pad_mode, c.T_out)
        return acc.reshape(1, M, N), mag.reshape(1, M, N)
    a64 = a_of(P["a_nat"])
    b64 = w_of(P["b_nat"])
    a64 = a64 if P["na"] == nz else a64[0]
    return torch.matmul(a64, b64.transpose(1, 2)), torch.matmul(a64.abs(), b64.abs().transpose(1, 2))


class _Device:
    """The problem's operands on the GPU, uploaded once for the launches of both engines."""
    def __init__(self, P):
        dev = lambda t: None if t is None else t.cuda()
        self.t = {k: dev(P[k]) for k in ("A", "A2", "Bw", "bias", "R", "gamma")}


def _launch(P, D, engine, epi, out):
    """One probe launch; returns (form, output buffers as CPU tensors, pitch, zC).  Every output word starts as a NaN pattern."""
    from wavtokenizer_amd import _capi
    nz, M, N, K, c = P["nz"], P["M"], P["N"], P["K"], P["c"]
    d = _capi.WtGemmDesc()
    d.size = ctypes.sizeof(d)
    d.engine, d.epi, d.out, d.pro = engine, epi, out, G.PRO_NONE
    d.b_is_act = 1 if c.b_act else 0
    d.M, d.N, d.K, d.nz, d.alpha = M, N, K, nz, ALPHA
    d.stride, d.dil, d.taps = 1, 1, 1
    for k, v in P["fields"].items():
        setattr(d, k, v)
    pitch = _r(N, 32) + 32
    zC = (M + 2) * pitch + 32
    d.c_rstride, d.zC = pitch, zC
    bufs = [torch.full((nz * zC,), 0x7FC00000 if out == G.OUT_F32 else 0x7E007E00, dtype=torch.int32).cuda()]    # (the eight pairs write C alone)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    t = D.t
    p = lambda x: x.data_ptr() if x is not None else None
    d.A, d.A2, d.B, d.bias, d.R, d.gamma = p(t["A"]), p(t["A2"]), p(t["Bw"]), p(t["bias"]), p(t["R"]), p(t["gamma"])
    d.C = bufs[0].data_ptr()
    d.status = status.data_ptr()
    nws = _capi.lib.wt_gemm_probe_workspace_bytes(ctypes.byref(d))
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    form = _capi.WtLaunchForm()
    rc = _capi.lib.wt_gemm_probe(ctypes.byref(d), ctypes.byref(form), _ptr(ws), None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    assert int(status[0]) == 0, f"range status {int(status[0])} on an in-range problem"
    return form, [b.cpu() for b in bufs], pitch, zC


def _logical(buf, out, nz, M, N, pitch, zC):
    """The logical [nz][M][N] region of an output buffer as float64."""
    if out == G.OUT_F32:
        return buf.view(torch.float32).reshape(nz, zC)[:, : M * pitch].reshape(nz, M, pitch)[:, :, :N].double()
    h = buf.view(torch.int16)
    return torch.stack([G.decode_s32_rows(h[2 * z * zC: 2 * z * zC + 2 * M * pitch], M, N) for z in range(nz)])


def _form_tuple(f):
    return (f.BM, f.BN, f.waves_m, f.waves_n, f.stages, f.ks, f.prod, f.staged, f.bias_cache, f.G, f.tiles)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS16H, ids=_ids)
def test_twin_runs_every_form_with_the_bits_of_the_default_on_f16_exact_operands(pair):
    epi, out = pair
    forms = set()
    for i, c in enumerate(_cases16(epi, out, _ncu())):
        P = _problem(epi, c, seed=1000 * epi + 10 * out + i, mode="f16")
        D = _Device(P)
        f0, b0, _p, _z = _launch(P, D, 0, epi, out)
        f2, b2, _p, _z = _launch(P, D, 2, epi, out)
        assert _form_tuple(f2) == _form_tuple(f0), (i, dict(c), _form_tuple(f2), _form_tuple(f0))
        for x0, x2 in zip(b0, b2):
            diff = int((x0 != x2).sum())
            assert diff == 0, f"case {i} {dict(c)} on {_form_name(f2)}: {diff} words differ from the three-product kernel's"
        forms.add(_form_name(f2))
    print(f"gemm16h {_ids(pair)}: forms {sorted(forms)}")
    assert forms == (EXPECT16_HEAD if epi == G.EPI_HEAD else EXPECT16), forms


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS16H, ids=_ids)
def test_twin_is_within_the_bound_of_the_hi_half_product(pair):
    epi, out = pair
    worst = 0.0
    for i, c in enumerate(_cases16(epi, out, _ncu())):
        P = _problem(epi, c, seed=2000 * epi + 10 * out + i, mode="general")
        w_of = f16_ref.act_hi if c.b_act else f16_ref.weight_hi        # an activation B operand is split unscaled
        acc, mag = _products(P, f16_ref.act_hi, w_of)
        dbl = lambda t: None if t is None else t.double()
        R = None if P["R"] is None else P["R"].double()[:, :P["N"]]
        refs, bounds = G.epilogue(epi, out, acc, mag, bias=dbl(P["bias"]), R=R, gamma=dbl(P["gamma"]),
                                  alpha=float(np.float32(ALPHA)), head_kb=P["N"] // 2)
        _f, bufs, pitch, zC = _launch(P, _Device(P), 2, epi, out)
        nz, M, N = P["nz"], P["M"], P["N"]
        got = _logical(bufs[0], out, nz, M, N, pitch, zC)
        ref, bnd = refs[0], bounds[0]
        nbad, frac, finite = G.check(got, ref.expand(nz, M, N) if ref.shape[0] != nz else ref,
                                     bnd.expand(nz, M, N) if bnd.shape[0] != nz else bnd)
        assert finite, f"case {i} {dict(c)}: an element of the logical region was not written (or is not finite)"
        assert nbad == 0, f"case {i} {dict(c)}: {nbad} elements outside the bound (worst {frac:.3g} x bound)"
        worst = max(worst, frac)
    print(f"gemm16h {_ids(pair)}: worst error {worst:.3g} of the bound around the hi-half product")


@pytest.mark.gpu
def test_the_mode_is_in_effect():
    """Operands uniform in [1, 2): every lo half is non-zero.  Against the float64 product of the unrounded operands the twin's
    RMS error must be at least 10 x the default kernel's (f16 rounding 2^-12 against the split form's 2^-22: about 2^10)."""
    epi, out = G.EPI_BIAS, G.OUT_F32
    c = lin(300, 96, 160)                          # (a weight maximum below 2 keeps the scale 1)
    P = _problem(epi, c, seed=5, mode="unit")
    ident = lambda t: t.double()
    acc, _mag = _products(P, ident, ident)
    ref = acc + P["bias"].double()
    D = _Device(P)
    rms = {}
    for engine in (0, 2):
        _f, bufs, pitch, zC = _launch(P, D, engine, epi, out)
        got = _logical(bufs[0], out, 1, P["M"], P["N"], pitch, zC)
        rms[engine] = float(((got - ref) ** 2).mean().sqrt())
    print(f"RMS error against float64: three products {rms[0]:.3e}, one product {rms[2]:.3e}, ratio {rms[2] / rms[0]:.1f}")
    assert rms[2] >= 10.0 * rms[0], rms


@pytest.mark.parametrize("what,kw,msg", [
    ("an encoder-only pair", dict(engine=2, epi=G.EPI_BIAS_ELU, out=G.OUT_S32), "unsupported epilogue / output-format pair"),
    ("a mixed-length launch", dict(engine=2, mix_geom=8 * FAKE, pad_mode=1, Tp=64), "unsupported epilogue / output-format pair"),
    ("engine 3", dict(engine=3), "engine is"),
])
def test_probe_refuses_what_the_twin_does_not_exist_for(what, kw, msg):
    """Before any HIP call: the pointers are stand-ins (tests/test_gemm_checks.py), so this runs on a host without a GPU."""
    from wavtokenizer_amd import _capi
    d = _desc(**kw)
    assert _capi.lib.wt_gemm_probe(ctypes.byref(d), None, ctypes.c_void_p(7 * FAKE), None) == -1, what
    assert msg in _capi.lib.wt_last_error().decode(), (what, _capi.lib.wt_last_error())
    d0 = _desc(**dict(kw, engine=2)) if what == "engine 3" else None
    if d0 is not None:       # ... while engine 2 itself is known: the same descriptor passes every check up to the first HIP call
        assert _capi.lib.wt_gemm_probe_workspace_bytes(ctypes.byref(d0)) > 0
