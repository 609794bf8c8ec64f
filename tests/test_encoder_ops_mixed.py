"""The mixed-length encoder kernels (resblock16_mixed_kernel, gemm16s_mixed_kernel, mixed_geometry_kernel: the launches of a
WT_PLAN_FLAG_MIXED_LENGTH plan), one launch at a time through wt_resblock_probe, wt_gemm_probe and wt_geometry_probe with a
geometry table.  Per family: a clip's rows up to its own length pass the float64 bound of tests/enc_ref.py (the GEMMs:
tests/gemm_ref.py) computed for that clip alone, are the bits of the one-length probe of that clip alone, and hold no NaN
although everything past a clip's length in the inputs is NaN; output rows past a clip's length keep their NaN prefill
(resblock16) or are finite (gemm16s); the guard words are intact, the status word is clear and the launch reports its form.
The last test compares the instantiations the session reached with the ones the launchers can pick."""
import ctypes

import pytest
import torch

from oracle.cpu_ref import get_extra_padding_for_conv1d
from tests import enc_ref as E
from tests import gemm_ref as G
from tests import parity_log
from tests.test_encoder_ops import DOWN, NAN_BITS, Out, check, check_form, decode, ncu, run_rb, weights
from tests.util import synth_state_dict

pytestmark = pytest.mark.gpu

HIT = set()
WORST = {}
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ geometry
def geom_words(n_stages):
    from wavtokenizer_amd import _capi
    w = _capi.WtGeomWords()
    assert _capi.lib.wt_geometry_words(n_stages, ctypes.byref(w)) == 0
    return w


def geometry(lengths, Tpad, tmin, kd, rd, kf):
    """The device table [B][words] (int32) of a chain, through the plans' geometry launch."""
    from wavtokenizer_amd import _capi
    w = geom_words(len(kd))
    B = len(lengths)
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    out = Out(B * w.words)
    d = _capi.WtGeomDesc()
    d.size = ctypes.sizeof(d)
    d.B, d.tmin, d.n_stages, d.kf, d.Tpad = B, tmin, len(kd), kf, Tpad
    for i, (k, r) in enumerate(zip(kd, rd)):
        d.kd[i], d.rd[i] = k, r
    d.lengths, d.geom = lens.data_ptr(), out.ptr
    assert _capi.lib.wt_geometry_probe(ctypes.byref(d), None) == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    out.host()                                            # guard words
    return out, w


def chain_of(arch):
    from wavtokenizer_amd.config import NAMED_ARCHS
    rd = list(NAMED_ARCHS[arch].enc_ratios)
    return [2 * r for r in rd], rd, 7


def sconv_geometry(T, k, stride):
    """{T_in, Tp, T_out} by the arithmetic of conv.py:54-61, 86-91, 195-211 (oracle.cpu_ref), cross-checked with wt_sconv_geometry."""
    from wavtokenizer_amd import _capi
    pt = k - stride
    extra = get_extra_padding_for_conv1d(T, k, stride, pt)
    pr = pt // 2
    pl = pt - pr
    Tout = (T + pt + extra - k) // stride + 1
    Tp = max(T, max(pl, pr + extra) + 1)
    o = (ctypes.c_int32 * 4)()
    assert _capi.lib.wt_sconv_geometry(T, k, stride, 1, o) == 0
    assert list(o) == [pl, pr + extra, Tout, Tp], (T, k, stride, list(o))
    return [T, Tp, Tout]


@pytest.mark.parametrize("arch", ["hop600", "hop320"])
def test_geometry_table(arch):
    """Every word of the table for lengths across [tmin, Tpad] and on both invalid sides."""
    kd, rd, kf = chain_of(arch)
    tmin, Tpad = 1024, 72000
    lengths = [tmin, tmin + 1, 1027, 1080, 1117, 2399, 2400, 2401, 24000, 61920, Tpad - 1, Tpad, tmin - 1, 1, 0, -5, Tpad + 1, 2 ** 31 - 1]
    out, w = geometry(lengths, Tpad, tmin, kd, rd, kf)
    got = out.host().reshape(len(lengths), w.words)
    want = torch.zeros_like(got)
    for b, T in enumerate(lengths):
        valid = tmin <= T <= Tpad
        Tc = T if valid else tmin
        want[b, w.valid], want[b, w.T], want[b, w.Tread] = int(valid), Tc, Tc if valid else 0
        for s, (k, r) in enumerate(zip(kd, rd)):
            base = w.stage0 + s * w.stage_words
            want[b, base + w.c3:base + w.c3 + 3] = torch.tensor(sconv_geometry(Tc, 3, 1))
            want[b, base + w.sc:base + w.sc + 3] = torch.tensor(sconv_geometry(Tc, 1, 1))
            dn = sconv_geometry(Tc, k, r)
            want[b, base + w.down:base + w.down + 3] = torch.tensor(dn)
            Tc = dn[2]
        want[b, w.final_conv:w.final_conv + 3] = torch.tensor(sconv_geometry(Tc, kf, 1))
        want[b, w.L] = Tc
    assert torch.equal(got, want), (got != want).nonzero()[:8]


# ------------------------------------------------------------------------------------------------ resblock16, mixed
def _mixed_resblock(r, lengths, Tpad, seed, tmin=1024):
    """r = 2 / 4: the fused stage-1 kernel with its down conv; r = 0: the plain C = 64 block on the frames stage 1 leaves."""
    arch = DOWN[r] if r else "hop600"
    kd, rd, kf = chain_of(arch)
    table, w = geometry(lengths, Tpad, tmin, kd, rd, kf)
    B = len(lengths)
    gen = torch.Generator().manual_seed(seed)
    valid = [tmin <= T <= Tpad for T in lengths]
    if r:
        W, D = weights(arch, 1)
        C, Tk, own = 32, Tpad, [T if v else tmin for T, v in zip(lengths, valid)]
        full = torch.randn(B, Tpad, generator=gen).float().double()
        inp = full.clone()
        for b in range(B):
            inp[b, own[b] if valid[b] else 0:] = NAN           # an invalid clip is never read
        mix = (table.ptr + 4 * w.T, table.ptr + 4 * w.Tread)
        rows_of = lambda T: -(-T // r)
        f, words = run_rb(D, B, Tk, C, wav=inp, r=r, mix=mix)
        opt = (126 - 2 * r) // r + 1
        check_form(f, 1, 32, 1, r, 32, B * -(-rows_of(Tk) // opt), hit=set())
    else:
        W, D = weights(arch, 4)
        r0 = rd[0]
        C, Tk, own = 64, -(-Tpad // r0), [-(-(T if v else tmin) // r0) for T, v in zip(lengths, valid)]
        full = torch.randn(B, C, Tk, generator=gen).float().double()
        inp = full.clone()
        for b in range(B):
            inp[b, :, own[b]:] = NAN                           # (an invalid clip's rows up to tmin's frames come from stage 1)
        word = w.stage0 + w.stage_words + w.c3                 # stage 2's k3 conv: T_in
        mix = (table.ptr + 4 * word, table.ptr + 4 * word)
        rows_of = lambda T: T
        f, words = run_rb(D, B, Tk, C, x=inp, elu_out=1, out_s32=1, mix=mix)
        check_form(f, 1, 64, 0, 0, 16, B * -(-Tk // 128), hit=set())
    HIT.add((r, "wrapped") if f.grid < f.tiles else (r,))
    ch = words.shape[-1]
    for b in range(B):
        n = rows_of(own[b])
        assert bool((words[b, n:] == NAN_BITS).all()), f"clip {b}: rows past its length were written"
        got = decode(words[b, :n], 0 if r else 1).reshape(1, n, ch)
        assert bool(torch.isfinite(got).all()), f"clip {b}: padding was read"
        if not valid[b]:
            continue
        if r:
            clip = dict(wav=full[b:b + 1, :own[b]])
            fs, solo = run_rb(D, 1, own[b], C, r=r, **clip)
            ref, bound = E.resblock(W, down=r, **clip)
        else:
            clip = dict(x=full[b:b + 1, :, :own[b]])
            fs, solo = run_rb(D, 1, own[b], C, elu_out=1, out_s32=1, **clip)
            ref, bound = E.resblock(W, elu_out=1, out_s32=1, **clip)
        assert fs.kernel == 0
        assert torch.equal(words[b, :n], solo[0]), f"clip {b} (length {lengths[b]}): not the bits of the one-length launch"
        check(got, ref, bound, f"mixed r={r} clip {b} length {lengths[b]}", f"resblock16 mixed {'down r=%d' % r if r else 'c64'}", WORST)
    return f


# lengths (samples): the shortest allowed, Tpad, a shifted last tile (no multiple of the stride), whole tiles past the clip, an
# exact number of output tiles, one invalid length on either side
@pytest.mark.parametrize("r,Tpad,lengths", [
    (4, 1500, [1024, 1500, 1027, 1100, 1000, 1080, 1501, 1203]),
    (2, 1400, [1024, 1400, 1025, 1116, 1023, 1117, 1401, 1241]),
    (0, 1500, [1024, 1500, 1027, 1100, 1000, 1280, 1501, 1029]),
])
def test_resblock16_mixed(r, Tpad, lengths):
    f = _mixed_resblock(r, lengths, Tpad, seed=Tpad + r)
    assert f.grid == f.tiles


@pytest.mark.parametrize("r", [4, 2, 0])
def test_resblock16_mixed_wrapped_grid(r):
    """More tiles than resident workgroups with two short clips among five: tiles wholly past a clip are skipped inside the
    persistent loop (with the waveform window of the next computed tile taken from the right buffer)."""
    arch = DOWN[r] if r else "hop600"
    _W, D = weights(arch, 1 if r else 4)
    if r:
        f0, _ = run_rb(D, 1, 1024, 32, wav=torch.zeros(1, 1024, dtype=torch.float64), r=r)
    else:
        f0, _ = run_rb(D, 1, 4, 64, x=torch.zeros(1, 64, 4, dtype=torch.float64))
    slots = ncu() * min(4, 160 * 1024 // f0.lds)       # resident workgroups, as the launchers count them
    if r:
        opt = (126 - 2 * r) // r + 1
        Tpad = opt * r * (slots // 5 + 2) - 1
    else:
        Tpad = 128 * 4 * (slots // 5 + 2) - 2
    f = _mixed_resblock(r, [Tpad, 1024, Tpad - 601, 1024, Tpad // 2 + 3], Tpad, seed=r)
    assert f.grid < f.tiles, (f.grid, f.tiles)


# ------------------------------------------------------------------------------------------------ gemm16s, mixed
PAIRS = [(G.EPI_BIAS, G.OUT_S32_DUAL_ELU), (G.EPI_BIAS, G.OUT_F32_AND_S32), (G.EPI_BIAS_ELU, G.OUT_S32)]       # WT_GEMM16S_MIXED_PAIRS
FMTS = {G.OUT_S32: ["s32"], G.OUT_S32_DUAL_ELU: ["s32", "s32"], G.OUT_F32_AND_S32: ["f32", "s32"]}
STAGE_OF_C = {64: 4, 128: 7, 256: 10}
_CONVS = {}


def conv_weights(kind, arch, C):
    """(w [N][Cin][k] float64 of fp32 values, bias [N], stride) of one of the encoder's own convs: the k3 conv C -> C / 2, the
    shortcut + conv1 [Ws | W1] over [x | elu(h)], the stage's down conv C -> 2 C, the final k7 conv."""
    key = (kind, arch, C)
    if key not in _CONVS:
        sd = synth_state_dict(arch)
        conv = lambda i, n: (E.fold_weight_norm(sd[E.ENC + f"{i}.{n}.weight_g"], sd[E.ENC + f"{i}.{n}.weight_v"]),
                             torch.as_tensor(sd[E.ENC + f"{i}.{n}.bias"]).double())
        if kind == "final":
            w, b = conv(15, "conv.conv")
            _CONVS[key] = (w, b, 1)
        else:
            st = STAGE_OF_C[C]
            if kind == "k3":
                w, b = conv(st, "block.1.conv.conv")
                _CONVS[key] = (w, b, 1)
            elif kind == "sc":
                (ws, bs), (w1, b1) = conv(st, "shortcut.conv.conv"), conv(st, "block.3.conv.conv")
                _CONVS[key] = (torch.cat([ws, w1], 1), bs + b1, 1)
            else:
                w, b = conv(st + 2, "conv.conv")
                _CONVS[key] = (w, b, w.shape[-1] // 2)
    return _CONVS[key]


def gemm_launch(A, A2, w, bias, stride, tap_pair, epi, out, mix=None):
    """One gemm16s probe launch of SConv1d(w) over A [clips][T_in][cols] (+ A2 [clips][T_in][cols2]: K columns past cols), host
    fp32: (form, [output words [clips][T_out][N] per output])."""
    from wavtokenizer_amd import _capi
    clips, T_in, cols = A.shape
    N, Cin, k = w.shape
    _t, Tp, T_out = sconv_geometry(T_in, k, stride)
    d = _capi.WtGemmDesc()
    d.size = ctypes.sizeof(d)
    d.engine, d.epi, d.out, d.pro, d.b_is_act = 0, epi, out, G.PRO_NONE, 0
    d.M, d.N, d.K, d.nz, d.alpha = clips * T_out, N, k * Cin, 1, 1.0
    d.T_in, d.T_out, d.Cin, d.taps, d.stride, d.dil = T_in, T_out, Cin, k, stride, 1
    d.pad_left, d.pad_mode, d.tap_pair, d.Tp = (k - stride) - (k - stride) // 2, 1, 1 if tap_pair else 0, Tp
    d.a_bstride, d.a_rstride, d.w_rstride, d.c_rstride = T_in * cols, cols, k * Cin, N
    order = G.tap_order(k, stride, tap_pair)
    keep = [A.float().contiguous().cuda(), w[:, :, order].permute(0, 2, 1).reshape(N, k * Cin).float().contiguous().cuda(),
            bias.float().cuda(), torch.zeros(4, dtype=torch.int32, device="cuda")]
    d.A, d.B, d.bias, d.status = (t.data_ptr() for t in keep)
    if A2 is not None:
        keep.append(A2.float().contiguous().cuda())
        d.A2, d.K1, d.a2_bstride, d.a2_rstride = keep[-1].data_ptr(), cols, T_in * A2.shape[2], A2.shape[2]
    outs = [Out(clips * T_out * N) for _ in FMTS[out]]
    d.C = outs[0].ptr
    if len(outs) > 1:
        d.C2 = outs[1].ptr
    if mix is not None:
        d.mix_geom = mix
    ws = torch.empty(max(_capi.lib.wt_gemm_probe_workspace_bytes(ctypes.byref(d)), 256), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    form = _capi.WtLaunchForm()
    rc = _capi.lib.wt_gemm_probe(ctypes.byref(d), ctypes.byref(form), ctypes.c_void_p(ws.data_ptr()), None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    assert int(keep[3][0]) == 0, "range status on an in-range problem"
    return form, [o.host().reshape(clips, T_out, N) for o in outs]


def _mixed_gemm(kind, arch, C, lengths, Tpad, want_form, seed):
    w, bias, stride = conv_weights(kind, arch, C)
    N, Cin, k = w.shape
    B = len(lengths)
    tap_pair = kind == "down"
    # the table: this conv as the k3 / 1x1 / down conv of stage 0 of a one-stage chain, or as that chain's final conv
    if kind == "final":
        table, gw = geometry(lengths, Tpad, 1, [1], [1], k)
        word = gw.final_conv
    else:
        table, gw = geometry(lengths, Tpad, 1, [k if kind == "down" else 1], [stride], 7)
        word = gw.stage0 + {"k3": gw.c3, "sc": gw.sc, "down": gw.down}[kind]
    gen = torch.Generator().manual_seed(seed)
    cols = C if kind == "sc" else Cin
    full = torch.randn(B, Tpad, Cin, generator=gen).float().double()
    if kind == "sc":
        full[:, :, cols:] = G.elu(full[:, :, cols:])              # the second K source holds elu(h)
    inp = full.clone()
    for b, T in enumerate(lengths):
        inp[b, T:] = NAN
    split = (lambda t: (t[:, :, :cols], t[:, :, cols:])) if kind == "sc" else (lambda t: (t, None))
    refs = {}
    for b, T in enumerate(lengths):                               # float64, once per clip, shared by the pairs
        _t, _tp, To = sconv_geometry(T, k, stride)
        pt = k - stride
        refs[b] = (To,) + G.conv_ref(full[b:b + 1, :T].transpose(1, 2), w, stride, 1, pt - pt // 2, pt // 2 + get_extra_padding_for_conv1d(T, k, stride, pt), 1, To)
    for epi, out in PAIRS:
        f, outs = gemm_launch(*split(inp), w, bias, stride, tap_pair, epi, out, mix=table.ptr + 4 * word)
        name = f"{f.BM}x{f.BN}"
        assert name == want_form and (f.ks, f.prod, f.stages) == (1, 0, 3), (name, f.ks, f.prod, f.stages)
        HIT.add((epi, out, name))
        assert f.tiles == -(-B * sconv_geometry(Tpad, k, stride)[2] // f.BM) * -(-N // f.BN)
        if f.tiles <= (ncu() & ~7):                       # fewer tiles than resident workgroups: one workgroup per tile
            assert f.G == f.tiles, (f.G, f.tiles)
        for b, T in enumerate(lengths):
            To, acc, mag = refs[b]
            _fs, solo = gemm_launch(*split(full[b:b + 1, :T]), w, bias, stride, tap_pair, epi, out)
            ref, bound = G.epilogue(epi, out, acc, mag, bias=bias)
            for fmt, o, s, rf, bd in zip(FMTS[out], outs, solo, ref, bound):
                assert torch.equal(o[b, :To], s[0]), f"{kind} C={C} clip {b} (length {T}): not the bits of the one-length launch"
                check(decode(o[b, :To], fmt == "s32").reshape(1, To, N), rf, bd, f"{kind} {arch} C={C} {G.EPI_NAMES[epi]}/{G.OUT_NAMES[out]} clip {b} length {T}",
                      f"gemm16s mixed {kind}", WORST)
                assert bool(torch.isfinite(decode(o[b, To:], fmt == "s32")).all()), f"clip {b}: a row past its T_out is not finite"


SHORT = [1, 2, 3, 40, 17, 5, 33, 40, 7]          # several clips per row tile, boundaries inside a tile, the padded length itself


@pytest.mark.parametrize("kind,arch,C,lengths,Tpad,form", [
    ("k3", "hop600", 64, SHORT, 40, "256x64"),                   # N = 32
    ("k3", "hop600", 128, SHORT, 40, "256x64"),                  # N = 64
    ("k3", "hop320", 256, SHORT, 40, "128x64"),                  # N = 128
    ("sc", "hop600", 128, SHORT, 40, "128x64"),                  # K = 128 + 64 through A2
    ("sc", "hop320", 256, SHORT, 40, "128x64"),
    ("down", "hop320", 64, [1, 2, 3, 50, 17, 9, 33, 50, 47], 50, "128x64"),      # r = 4, k = 8, paired taps
    ("down", "hop600", 64, [1, 2, 3, 50, 17, 9, 33, 50, 46], 50, "128x64"),      # r = 5
    ("down", "hop600", 256, [1, 2, 3, 50, 17, 11, 33, 50, 49], 50, "128x64"),    # r = 6
    ("down", "hop320", 256, [1, 2, 3, 50, 17, 15, 33, 50, 41], 50, "128x64"),    # r = 8
    ("final", "hop600", 512, [1, 2, 3, 30, 17, 5, 30], 30, "128x64"),            # k7 512 -> 512
    ("sc", "hop600", 128, [1601, 3, 1500, 1601, 2, 1333, 1601, 1, 777], 1601, "128x128"),   # more than 100 tiles of 128 x 128
])
def test_gemm16s_mixed(kind, arch, C, lengths, Tpad, form):
    _mixed_gemm(kind, arch, C, lengths, Tpad, form, seed=C + Tpad)


def test_every_instantiation_was_reached():
    """Runs last: the three mixed resblock16 instantiations, each also with a wrapped grid, and every pair of
    WT_GEMM16S_MIXED_PAIRS on every tile form launch16s_mixed can pick; the worst fraction of the bound per family goes to the
    parity log."""
    for fam, w in sorted(WORST.items()):
        parity_log.record(f"encoder_ops_mixed {fam}", worst_of_bound=w)
    want = {(r,) for r in (0, 2, 4)} | {(r, "wrapped") for r in (0, 2, 4)}
    want |= {(e, o, f) for e, o in PAIRS for f in ("256x64", "128x64", "128x128")}
    assert HIT == want, HIT ^ want
