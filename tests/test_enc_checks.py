"""CPU-only halves of tests/test_encoder_ops.py and tests/test_encoder_ops_mixed.py: the bounds of tests/enc_ref.py are honest
(an fp32 evaluation in two summation orders and a simulated split-f16 evaluation stay inside them on every element) and sharp
(each slip an encoder kernel could make puts at least one element outside them), at shapes the GPU files use.  The evaluator
here is written on index arithmetic, independently of enc_ref's (which pads through the oracle's helpers)."""
import pytest
import torch

from tests import enc_ref as E
from tests import gemm_ref as G
from tests.util import synth_state_dict


# ------------------------------------------------------------------------------------------------ the evaluator
def _mm(mode):
    """A [.., K] x W [N][K] -> [.., N] in the arithmetic `mode` names."""
    if mode == "f64":
        return lambda A, W: A @ W.t()
    if mode == "f32":                    # torch's blocked fp32 product
        return lambda A, W: (A.float() @ W.float().t()).double()
    if mode == "f32rev":                 # one strictly serial fp32 chain, K descending
        def serial(A, W):
            A, W = A.float(), W.float()
            acc = torch.zeros(A.shape[:-1] + (W.shape[0],), dtype=torch.float32)
            for k in range(A.shape[-1] - 1, -1, -1):
                acc = acc + A[..., k:k + 1] * W[:, k]
            return acc.double()
        return serial
    if mode in ("s16", "s16_nolo_w", "s16_nolo_a"):      # hi + lo 2^-11 operands, lo.lo dropped, fp32 accumulation
        def split(v):
            hi = v.float().half().float()
            lo = ((v.float() - hi) * 2048.0).half().float()
            return hi, lo
        def prod(A, W):
            ah, al = split(A)
            wh, wl = split(W)
            if mode == "s16_nolo_w":     # the lo half of the weights dropped
                wl = torch.zeros_like(wl)
            if mode == "s16_nolo_a":     # ... of the activations
                al = torch.zeros_like(al)
            return ((ah @ wh.t()) + ((al @ wh.t()) + (ah @ wl.t())) * (1.0 / 2048.0)).double()
        return prod
    raise ValueError(mode)


def _tmap(T, k, stride, slip=None):
    """[Tout][k] source frame of every tap of SConv1d over T frames (-1: a zero), by the arithmetic of conv.py:54-61, 79-96."""
    pt = k - stride
    pr = pt // 2
    pl = pt - pr
    Tout = -(-T // stride)
    extra = (Tout - 1) * stride + k - pt - T
    Tp = max(T, max(pl, pr + extra) + 1)
    p = torch.arange(Tout)[:, None] * stride + torch.arange(k)[None, :]         # padded coordinate
    pos = p - pl
    pos = torch.where(pos < 0, -pos, pos)
    if slip == "refl_2T-1":
        pos = torch.where(pos >= Tp, 2 * Tp - 1 - pos, pos)
    elif slip == "zero_past_clip":
        pos = torch.where(pos >= T, torch.full_like(pos, -1), pos)
    else:
        pos = torch.where(pos >= Tp, 2 * (Tp - 1) - pos, pos)
    pos = torch.where(pos >= T, torch.full_like(pos, -1), pos)
    if slip == "no_extra_pad":
        pos = torch.where(p >= pl + T + pr, torch.full_like(pos, -1), pos)
    return pos


def _conv(x, w, b, tmap, mm, order=None):
    """x [B][Cin][Tbuf], w [N][Cin][k] -> [B][N][Tout] through the gather tmap; K runs tap-major as in the kernels."""
    B, Cin = x.shape[:2]
    N, _, k = w.shape
    cols = x[:, :, tmap.clamp(min=0)] * (tmap >= 0)                            # [B][Cin][Tout][k]
    order = list(range(k)) if order is None else order
    A = cols.permute(0, 2, 3, 1).reshape(B, tmap.shape[0], k * Cin)
    Wm = w[:, :, order].permute(0, 2, 1).reshape(N, k * Cin)
    return (mm(A, Wm) + b).transpose(1, 2)


def _elu(v, mode):
    if mode == "f64":
        return G.elu(v)
    f = v.float()
    return torch.where(f > 0, f, torch.expm1(f)).double()


CONTRACTIONS = ("first", "k3", "out", "down")


def chain(W, T, x=None, wav=None, down=0, elu_out=0, mode="f64", slip=None):
    """The fused block (enc_ref.resblock) on the first T frames of x [B][C][Tbuf] / wav [B][Tbuf], time-major result.
    slip: one deliberate mistake; "refl_2T-1@<contraction>": that conv reflects off by one at the clip end;
    "nolo_<w|a>@<contraction>" (mode s16): that contraction alone loses the lo half of its weights / activations."""
    at = slip.split("@")[1] if slip and "@" in slip else None
    kind = slip.split("@")[0] if slip else None

    def mm_of(c):
        return _mm("s16_" + kind) if kind in ("nolo_w", "nolo_a") and at == c else _mm(mode)

    def refl(c):
        return "refl_2T-1" if kind == "refl_2T-1" and at == c else None
    Tl = (x if x is not None else wav).shape[-1] if slip == "reflect_at_Tpad" else T       # the length the index arithmetic uses
    if wav is not None:
        x = _conv(wav[:, None, :], W["e0w"], W["e0b"], _tmap(Tl, 7, 1, refl("first")), mm_of("first"))
    a = _elu(x, mode)
    h = _conv(a, W["w3"], W["b3"], _tmap(Tl, 3, 1, refl("k3")), mm_of("k3"))
    g = _elu(h, mode)
    sx = _elu(x, mode) if slip == "elu_on_shortcut" else x
    b12 = W["bs"] if slip == "no_b1" else W["b1"] + W["bs"]
    y = mm_of("out")(torch.cat([g, sx[:, :, :g.shape[-1]]], 1).transpose(1, 2), torch.cat([W["w1"][:, :, 0], W["ws"][:, :, 0]], 1)) + b12
    y = y.transpose(1, 2)
    if down:
        z = y if slip == "no_elu_before_down" else _elu(y, mode)
        dslip = slip if slip in ("zero_past_clip", "no_extra_pad") else refl("down")
        d = _conv(z, W["wd"], W["bd"], _tmap(Tl, 2 * down, down, dslip), mm_of("down"))
        return d.transpose(1, 2)[:, :-(-T // down)]
    if elu_out:
        y = _elu(y, mode)
    return y.transpose(1, 2)[:, :T]


# ------------------------------------------------------------------------------------------------ the families
_W = {}


def weights(arch, stage):
    key = (arch, stage)
    if key not in _W:
        _W[key] = E.stage_weights(synth_state_dict(arch), stage, down=3 if stage == 1 else None)
    return _W[key]


def _inputs(fam, T, Tbuf=None, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + T)
    Tbuf = Tbuf or T
    if fam["fold"]:
        return dict(wav=torch.randn(3, Tbuf, generator=gen).float().double())
    return dict(x=torch.randn(3, fam["C"], Tbuf, generator=gen).float().double())


FAMILIES = {
    "c32_fold": dict(arch="hop600", stage=1, C=32, fold=True, down=0, Ts=[3, 129]),
    "c32_plain": dict(arch="hop600", stage=1, C=32, fold=False, down=0, Ts=[3, 129]),
    "c64": dict(arch="hop600", stage=4, C=64, fold=False, down=0, Ts=[3, 129]),
    "down_r4": dict(arch="hop600", stage=1, C=32, fold=True, down=4, Ts=[1025, 1030]),
    "down_r2": dict(arch="hop320", stage=1, C=32, fold=True, down=2, Ts=[1025, 1030]),
}


def _ref(fam, inp, T, chain_=E.S16, elu_out=0, out_s32=0):
    W = weights(fam["arch"], fam["stage"])
    cut = {k: v[..., :T] for k, v in inp.items()}
    return E.resblock(W, elu_out=elu_out, out_s32=out_s32, down=fam["down"], chain=chain_, **cut)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_bounds_accept_honest_evaluations(name):
    """fp32 in two summation orders inside both bounds, simulated split-f16 inside the split-f16 bound, on every element."""
    fam = FAMILIES[name]
    W = weights(fam["arch"], fam["stage"])
    for T in fam["Ts"]:
        inp = _inputs(fam, T)
        for elu_out in ((0, 1) if not fam["down"] else (0,)):
            for ch, modes in ((E.S16, ("f32", "f32rev", "s16")), (E.F32, ("f32", "f32rev"))):
                if ch is E.F32 and fam["down"]:
                    continue                     # resblock.hip has no down conv
                ref, bound = _ref(fam, inp, T, ch, elu_out)
                for mode in modes:
                    got = chain(W, T, down=fam["down"], elu_out=elu_out, mode=mode, **inp)
                    bad, worst, finite = G.check(got, ref, bound)
                    assert finite and bad == 0, (name, T, ch.name, mode, elu_out, worst)
        exact = chain(W, T, down=fam["down"], mode="f64", **inp)
        ref, bound = _ref(fam, inp, T)
        assert G.check(exact, ref, bound)[1] < 1e-3, "the two float64 evaluations disagree"


def _slips(fam):
    """The slips a family can make: the off-by-one reflection at every conv that reflects, the lo half of one operand of one
    contraction dropped, and the structural ones."""
    convs = [c for c in CONTRACTIONS if (c != "first" or fam["fold"]) and (c != "down" or fam["down"])]
    s = [f"refl_2T-1@{c}" for c in convs if c != "out"]
    s += [f"nolo_{o}@{c}" for c in convs for o in "wa"]
    s += ["no_b1", "elu_on_shortcut"]
    if fam["down"]:
        s += ["zero_past_clip", "no_extra_pad", "no_elu_before_down"]
    return s


@pytest.mark.parametrize("name", list(FAMILIES))
def test_bounds_reject_each_slip(name):
    """The reflection 2T - 1 - pos instead of 2 (T - 1) - pos at each conv that reflects, the lo half of the weights or of the
    activations dropped in one contraction, b1 dropped, ELU on the shortcut path; DOWN: a last window that sees zeros past the
    clip, the extra right padding dropped, ELU missing before the down conv.  Each one leaves at least one element outside the
    bound at every length it can show at."""
    fam = FAMILIES[name]
    W = weights(fam["arch"], fam["stage"])
    for T in fam["Ts"]:
        inp = _inputs(fam, T, seed=1)
        ref, bound = _ref(fam, inp, T)
        for slip in _slips(fam):
            if slip == "no_extra_pad" and T % fam["down"] == 0:
                continue                             # no extra padding to drop
            wrong = chain(W, T, down=fam["down"], mode="s16" if slip.startswith("nolo") else "f64", slip=slip, **inp)
            assert G.check(wrong, ref, bound)[0] > 0, (name, T, slip)


@pytest.mark.parametrize("name,T,Tpad", [("c64", 100, 130), ("c64", 129, 256), ("down_r4", 1030, 1200), ("down_r2", 1025, 1100)])
def test_bounds_reject_reflection_at_the_padded_length(name, T, Tpad):
    """A mixed-length kernel that reflects (and bounds its reads) at Tpad instead of the clip's own length reads what lies past
    the clip instead of the clip's reflected frames."""
    fam = FAMILIES[name]
    W = weights(fam["arch"], fam["stage"])
    inp = _inputs(fam, T, Tbuf=Tpad, seed=2)
    ref, bound = _ref(fam, inp, T)
    ok = chain(W, T, down=fam["down"], mode="f32", **inp)
    assert G.check(ok, ref, bound)[0] == 0
    wrong = chain(W, T, down=fam["down"], mode="f64", slip="reflect_at_Tpad", **inp)
    assert G.check(wrong, ref, bound)[0] > 0


# ------------------------------------------------------------------------------------------------ the GEMM gathers
def _gemm_case(Cin, N, k, stride, T, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(3, Cin, T, generator=gen).float().double()
    w = (torch.randn(N, Cin, k, generator=gen) / (Cin * k) ** 0.5).float().double()
    b = torch.randn(N, generator=gen).float().double()
    pt = k - stride
    pr = pt // 2
    Tout = -(-T // stride)
    extra = (Tout - 1) * stride + k - pt - T
    acc, mag = G.conv_ref(x, w, stride, 1, pt - pr, pr + extra, 1, Tout)
    (ref,), (bound,) = G.epilogue(G.EPI_BIAS, G.OUT_F32, acc, mag, bias=b)
    return x, w, b, ref, bound


@pytest.mark.parametrize("Cin,N,k,stride,T", [(64, 32, 3, 1, 5), (64, 128, 8, 4, 37), (128, 256, 10, 5, 23), (512, 512, 7, 1, 3)])
def test_gemm_bound_rejects_gather_slips(Cin, N, k, stride, T):
    """The per-clip conv bound of the mixed gemm16s cases (gemm_ref.conv_ref + epilogue): honest fp32 and split-f16 inside;
    outside: a clip's first frame taken from its neighbour's last frame, the paired tap order swapped, the lo half dropped."""
    x, w, b, ref, bound = _gemm_case(Cin, N, k, stride, T, seed=Cin + k)
    tmap = _tmap(T, k, stride)
    for mode in ("f32", "f32rev", "s16"):
        got = _conv(x, w, b, tmap, _mm(mode)).transpose(1, 2)
        bad, worst, finite = G.check(got, ref, bound)
        assert finite and bad == 0, (mode, worst)
    assert G.check(_conv(x, w, b, tmap, _mm("s16_nolo_w")).transpose(1, 2), ref, bound)[0] > 0
    if k - stride - (k - stride) // 2 > 0:
        # rows of a tile are consecutive frames of consecutive clips: position -1 of clip b is clip b - 1's last frame
        flat = x.transpose(0, 1).reshape(1, Cin, 3 * T)
        pos = torch.arange(-(-T // stride))[:, None] * stride + torch.arange(k)[None, :] - (k - stride - (k - stride) // 2)
        wrong = []
        for c in range(3):
            m = torch.where((pos < 0) & (c > 0), pos + c * T, torch.where(tmap >= 0, tmap + c * T, tmap))
            wrong.append(_conv(flat, w, b, m, _mm("f64")))
        assert G.check(torch.cat(wrong).transpose(1, 2), ref, bound)[0] > 0
    if k == 2 * stride:
        order = G.tap_order(k, stride, True)
        assert G.check(_conv(x, w, b, tmap, _mm("f64"), order=order).transpose(1, 2), ref, bound)[0] > 0


# ---------------------------------------------------------------------------------------------- refusals
FAKE = 1 << 20


def test_probes_refuse_before_any_hip_call():
    """Bad descriptors come back as WT_ERR_INVALID with a message, before any device memory is touched."""
    import ctypes
    from wavtokenizer_amd import _capi
    lib = _capi.lib

    def rb(**kw):
        d = _capi.WtResblockDesc()
        d.size = ctypes.sizeof(d)
        d.B, d.T, d.C = 2, 64, 64
        for i, n in enumerate(("x", "w3", "b3", "w1", "b1", "ws", "bs", "y")):
            setattr(d, n, (i + 1) * FAKE)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw, msg in [(dict(size=8), "another size"), (dict(C=48), "C = 32 and 64"), (dict(wav=9 * FAKE, e0_w=FAKE, e0_b=FAKE), "C == 32"),
                    (dict(mix_T=FAKE), "both length words"), (dict(mix_T=FAKE, mix_Tread=FAKE, C=32), "plain C = 64 block only"),
                    (dict(r=4, wav=9 * FAKE, e0_w=FAKE, e0_b=FAKE, wd=FAKE, bd=FAKE, C=32, T=1000), "T >= 1024"),
                    (dict(r=3, wav=9 * FAKE, e0_w=FAKE, e0_b=FAKE, wd=FAKE, bd=FAKE, C=32, T=2000), "stride 2 or 4"),
                    (dict(fp32_chain=1, out_s32=1), "fp32 kernel"), (dict(x=FAKE + 4), "16-byte aligned"), (dict(y=None), "null argument")]:
        d = rb(**kw)
        assert lib.wt_resblock_probe(ctypes.byref(d), None, None) == _capi.WT_ERR_INVALID, kw
        assert msg in lib.wt_last_error().decode(), (kw, lib.wt_last_error())

    def geo(**kw):
        d = _capi.WtGeomDesc()
        d.size = ctypes.sizeof(d)
        d.B, d.tmin, d.n_stages, d.kf, d.Tpad = 2, 1024, 2, 7, 4096
        d.kd[0], d.rd[0], d.kd[1], d.rd[1] = 8, 4, 10, 5
        d.lengths, d.geom = FAKE, 2 * FAKE
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw, msg in [(dict(size=8), "another size"), (dict(n_stages=7), "encoder stages"), (dict(Tpad=100), "tmin <= Tpad"),
                    (dict(lengths=None), "device arrays"), (dict(kf=0), "final conv")]:
        d = geo(**kw)
        assert lib.wt_geometry_probe(ctypes.byref(d), None) == _capi.WT_ERR_INVALID, kw
        assert msg in lib.wt_last_error().decode(), (kw, lib.wt_last_error())
    d = geo()
    d.kd[1] = 3
    assert lib.wt_geometry_probe(ctypes.byref(d), None) == _capi.WT_ERR_INVALID
    words = _capi.WtGeomWords()
    assert lib.wt_geometry_words(0, ctypes.byref(words)) == _capi.WT_ERR_INVALID
    assert lib.wt_geometry_words(4, ctypes.byref(words)) == 0
    assert words.final_conv == words.stage0 + 4 * words.stage_words and words.L == words.final_conv + 3 and words.L < words.words

    # wt_gemm_desc.mix_geom: optional and last; a mixed launch exists for the encoder's reflect-padded pairs only
    g = _capi.WtGemmDesc()
    g.size = ctypes.sizeof(g)
    g.epi, g.out = G.EPI_BIAS, G.OUT_F32
    g.M, g.N, g.K = 64, 64, 64
    g.T_in = g.T_out = g.Tp = 64
    g.Cin, g.taps, g.stride, g.dil, g.nz, g.pad_mode = 64, 1, 1, 1, 1, 1
    g.a_rstride, g.w_rstride, g.c_rstride = 64, 64, 64
    g.A, g.B, g.C, g.mix_geom = FAKE, 2 * FAKE, 3 * FAKE, 4 * FAKE
    assert lib.wt_gemm_probe(ctypes.byref(g), None, ctypes.c_void_p(7 * FAKE), None) == _capi.WT_ERR_INVALID
    assert "mixed-length launches exist" in lib.wt_last_error().decode()
    g.engine = 1
    assert lib.wt_gemm_probe(ctypes.byref(g), None, ctypes.c_void_p(7 * FAKE), None) == _capi.WT_ERR_INVALID
    assert "mix_geom" in lib.wt_last_error().decode()
    g.engine, g.size = 0, _capi.WtGemmDesc.mix_geom.offset + 4
    assert lib.wt_gemm_probe(ctypes.byref(g), None, ctypes.c_void_p(7 * FAKE), None) == _capi.WT_ERR_INVALID
    assert "another size" in lib.wt_last_error().decode()
