"""Every (epilogue, output format) pair of gemm16s.hip and every (prologue, epilogue) pair of gemm.hip, at every tile form
its launcher picks, against float64 references built from the definitions (tests/gemm_ref.py), through wt_gemm_probe:
the plans' own launchers with the plans' operand splitting.  Per case: a per-element error bound (not only a relative L2),
the write contract (NaN-filled logical region all written and finite, sentinel-filled padding untouched except the
zeroed partial run of 4 that EPI_SCALE / EPI_BIAS_ROW document) and, on gemm16s, a clear range status word.  Per pair:
the union of launch forms the cases reached must be the forms its launcher can choose, so that a launcher change that
strands a form fails here instead of going uncovered.  The argmax epilogue has its own file
(tests/test_vq_ops.py, through wt_vq_probe: every partial candidate, code and feature word against tests/vq_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_ref as G
from tests import parity_log

pytestmark = pytest.mark.gpu

F32_SENTINEL = -559038737        # 0xDEADBEEF as int32: the fp32 padding
F16_SENTINEL = -16657            # 0xBEEF as int16: the S32 padding (per half)
F16_NAN = 0x7E00
STAGEABLE16 = {(G.EPI_BIAS, G.OUT_F32), (G.EPI_BIAS, G.OUT_S32), (G.EPI_BIAS, G.OUT_S32_DUAL_ELU), (G.EPI_BIAS, G.OUT_F32_AND_S32),
               (G.EPI_BIAS_ELU, G.OUT_S32), (G.EPI_BIAS_GELU, G.OUT_S32), (G.EPI_HEAD, G.OUT_S32)}
BIAS_OPTIONAL = {G.EPI_BIAS, G.EPI_BIAS_RES, G.EPI_BIAS_ELU, G.EPI_BIAS_RES_ELU, G.EPI_BIAS_GELU, G.EPI_BIAS_GAMMA_RES}
RAGGED_N = {G.EPI_SCALE, G.EPI_BIAS_ROW}      # gemm16s: any N (the partial last run of 4 is written as zeros)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ncu():
    from wavtokenizer_amd import _capi
    cu = ctypes.c_int32()
    assert _capi.lib.wt_device_info(torch.cuda.current_device(), ctypes.byref(cu), None, None) == 0
    return cu.value


def _r(x, m):
    return (x + m - 1) // m * m


def _cells(M, pitch, n0, n1):
    """Flat indices of columns [n0, n1) of rows [0, M) of a row-major array of row pitch `pitch`."""
    return (np.arange(M)[:, None] * pitch + np.arange(n0, n1)[None, :]).reshape(-1)


def _form_name(f):
    return f"{f.BM}x{f.BN}" + (f"ks2p{f.prod}" if f.ks == 2 else "")


class Case(dict):
    def __getattr__(self, k):
        return self.get(k)


def lin(M, N, K, **kw):
    return Case(kind="lin", M=M, N=N, K=K, **kw)


def conv(clips, T_in, Cin, N, k, stride=1, dil=1, pad_mode=1, pl=None, pr=None, **kw):
    keff = (k - 1) * dil + 1
    pl = (keff - stride) - (keff - stride) // 2 if pl is None else pl
    pr = (keff - stride) // 2 if pr is None else pr
    T_out = (T_in + pl + pr - keff) // stride + 1
    return Case(kind="conv", clips=clips, T_in=T_in, Cin=Cin, N=N, k=k, stride=stride, dil=dil, pad_mode=pad_mode, pl=pl, pr=pr,
                T_out=T_out, M=clips * T_out, K=k * Cin, **kw)


def _run(engine, epi, out, pro, c, seed):
    """One probe launch of case c; returns (form, [(worst fraction of the bound, ...)]) after every assertion."""
    from wavtokenizer_amd import _capi
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    head = epi == G.EPI_HEAD
    nz, M, N, K = c.nz or 1, c.M, c.N, c.K
    wscale = c.wscale or 1.0
    d = _capi.WtGemmDesc()
    d.size = ctypes.sizeof(d)
    d.engine, d.epi, d.out, d.pro = (0 if engine == 16 else 1), epi, out, pro
    d.b_is_act = 1 if c.b_act else 0
    d.M, d.N, d.K, d.nz, d.alpha = M, N, K, nz, 0.0883883
    d.stride, d.dil, d.taps = 1, 1, 1
    # ---- operands (fp32, as the kernel reads them), references in float64 from the same fp32 values
    if c.kind == "conv":
        x = (rnd(c.clips, c.Cin, c.T_in) / wscale).double()
        w = (rnd(N, c.Cin, c.k) / (c.Cin * c.k) ** 0.5 * wscale).float().double()
        x = x.float().double()
        acc, mag = G.conv_ref(x, w, c.stride, c.dil, c.pl, c.pr, c.pad_mode, c.T_out, pro)
        acc, mag = acc.reshape(1, M, N), mag.reshape(1, M, N)
        A = x.transpose(1, 2).contiguous().float().reshape(-1)
        order = G.tap_order(c.k, c.stride, c.tap_pair)
        Bw = w[:, :, order].permute(0, 2, 1).reshape(N, K).float().contiguous().reshape(-1)
        d.T_in, d.T_out, d.Cin, d.taps, d.stride, d.dil = c.T_in, c.T_out, c.Cin, c.k, c.stride, c.dil
        d.pad_left, d.pad_mode, d.tap_pair = c.pl, c.pad_mode, 1 if c.tap_pair else 0
        d.Tp = max(c.T_in, max(c.pl, c.pr) + 1) if c.pad_mode == 1 else c.T_in
        d.a_bstride, d.a_rstride, d.w_rstride = c.T_in * c.Cin, c.Cin, K
        A2 = None
    else:
        K1 = c.K1 or K
        arow = K1 + (c.apad or 0)
        na = 1 if c.shared else nz
        a_nat = (rnd(na, M, K) / wscale).float()
        if head:
            kb = N // 2
            lm = rnd(nz, kb, K) / K ** 0.5 * wscale
            ph = rnd(nz, kb, K) / K ** 0.5 * 2 * wscale
            b_nat = torch.stack([G.pack_head_rows(lm[z], ph[z]) for z in range(nz)]).float()
        else:
            b_nat = (rnd(nz, N, K) / K ** 0.5 * wscale).float()
        a64, b64 = a_nat.double(), b_nat.double()
        if pro == G.PRO_ELU:
            a64 = G.elu(a64)
        acc = torch.matmul(a64, b64.transpose(1, 2)) if na == nz else torch.matmul(a64[0], b64.transpose(1, 2))
        mag = torch.matmul(a64.abs(), b64.abs().transpose(1, 2)) if na == nz else torch.matmul(a64[0].abs(), b64.abs().transpose(1, 2))
        Abuf = torch.zeros(na, M, arow)
        Abuf[:, :, :K1] = a_nat[:, :, :K1]
        A = Abuf.reshape(-1)
        A2 = None
        if c.K1:
            A2 = a_nat[0, :, K1:].contiguous().reshape(-1)
            d.K1, d.a2_rstride = K1, K - K1
        Bw = b_nat.reshape(-1).contiguous()
        d.T_in = d.T_out = M
        d.Cin = K
        d.a_rstride, d.w_rstride = arow, K
        d.zA = 0 if c.shared else M * arow
        d.zW = N * K
    # ---- epilogue operands
    bias = R = gamma = None
    if epi == G.EPI_BIAS_ROW:
        bias = rnd(M).float()
    elif head:
        bias = torch.stack([G.pack_head_rows(torch.randn(N // 2, generator=gen) * 2 + 2, torch.randn(N // 2, generator=gen))]).reshape(-1).float()
    elif epi != G.EPI_SCALE and not c.no_bias:
        bias = rnd(N).float()
    r_pitch = _r(N, 4) + 32
    if epi in (G.EPI_BIAS_RES, G.EPI_BIAS_RES_ELU, G.EPI_BIAS_GAMMA_RES):
        R = rnd(M, r_pitch).float()
        d.r_rstride = r_pitch
    if epi == G.EPI_BIAS_GAMMA_RES:
        gamma = (torch.rand(N, generator=gen) + 0.25).float()
    if head:
        d.head_kb = N // 2
    refs, bounds = G.epilogue(epi, out, acc, mag, bias=None if bias is None else bias.double(),
                              R=None if R is None else R.double()[:, :N], gamma=None if gamma is None else gamma.double(),
                              alpha=float(np.float32(d.alpha)), head_kb=N // 2)
    # ---- outputs: NaN in the logical region, sentinels everywhere else (pad columns, rows past M, gaps between z slices)
    pitch = _r(N, 32) + 32
    zC = (M + 2) * pitch + 32
    d.c_rstride, d.zC = pitch, zC
    fmts = {G.OUT_F32: ["f32"], G.OUT_S32: ["s32"], G.OUT_S32_DUAL_ELU: ["s32", "s32"], G.OUT_F32_AND_S32: ["f32", "s32"]}[out]
    bufs, masks = [], []
    for f in fmts:
        t = torch.empty(nz * zC, dtype=torch.float32)
        if f == "f32":
            t.view(torch.int32).fill_(F32_SENTINEL)
            m = np.zeros((nz, zC), bool)
            m[:, _cells(M, pitch, 0, N)] = True
            t.view(torch.int32)[torch.from_numpy(m.reshape(-1))] = 0x7FC00000
        else:
            t.view(torch.int16).fill_(F16_SENTINEL)
            m = np.zeros((nz, 2 * zC), bool)
            m[:, : 2 * M * pitch] = np.tile(G.s32_logical_mask(M, pitch, N).reshape(-1), nz).reshape(nz, -1)
            t.view(torch.int16)[torch.from_numpy(m.reshape(-1))] = F16_NAN
        bufs.append(t.cuda())
        masks.append(m)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    dev = lambda t: None if t is None else t.cuda()
    Ad, A2d, Bd, biasd, Rd, gd = dev(A), dev(A2), dev(Bw), dev(bias), dev(R), dev(gamma)
    d.A, d.A2, d.B = Ad.data_ptr(), (A2d.data_ptr() if A2d is not None else None), Bd.data_ptr()
    d.bias = biasd.data_ptr() if biasd is not None else None
    d.R = Rd.data_ptr() if Rd is not None else None
    d.gamma = gd.data_ptr() if gd is not None else None
    d.C = bufs[0].data_ptr()
    d.C2 = bufs[1].data_ptr() if len(bufs) > 1 else None
    d.status = status.data_ptr()
    nws = _capi.lib.wt_gemm_probe_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    form = _capi.WtLaunchForm()
    rc = _capi.lib.wt_gemm_probe(ctypes.byref(d), ctypes.byref(form), _ptr(ws), None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    # ---- checks
    worst = []
    for f, t, m, ref, bnd in zip(fmts, bufs, masks, refs, bounds):
        h = t.cpu()
        if f == "f32":
            bits = h.view(torch.int32).numpy().reshape(nz, zC)
            pad = ~m
            expect = np.full(bits.shape, F32_SENTINEL, np.int64)
            if engine == 16 and epi == G.EPI_SCALE and N % 4:
                run = np.zeros((nz, zC), bool)
                run[:, _cells(M, pitch, N, _r(N, 4))] = True
                expect[run] = 0
            bad = np.nonzero(bits[pad] != expect[pad])[0]
            assert bad.size == 0, f"{bad.size} padding words written, e.g. flat index {np.nonzero(pad.reshape(-1))[0][bad[0]]}"
            got = h[: nz * zC].reshape(nz, zC)[:, : M * pitch].reshape(nz, M, pitch)[:, :, :N].double()
        else:
            halves = h.view(torch.int16).numpy().reshape(nz, 2 * zC)
            pad = ~m
            expect = np.full(halves.shape, F16_SENTINEL, np.int64)
            if engine == 16 and epi == G.EPI_BIAS_ROW and N % 4:
                run = np.zeros((nz, 2 * zC), bool)
                run[:, : 2 * M * pitch] = np.tile((G.s32_logical_mask(M, pitch, _r(N, 4)) & ~G.s32_logical_mask(M, pitch, N)).reshape(-1), nz).reshape(nz, -1)
                expect[run] = 0
            bad = np.nonzero(halves[pad] != expect[pad])[0]
            assert bad.size == 0, f"{bad.size} padding halves written"
            got = torch.stack([G.decode_s32_rows(h.view(torch.int16)[2 * z * zC: 2 * z * zC + 2 * M * pitch], M, N) for z in range(nz)])
        nbad, frac, finite = G.check(got, ref.expand(nz, M, N) if ref.shape[0] != nz else ref, bnd.expand(nz, M, N) if bnd.shape[0] != nz else bnd)
        assert finite, "an element of the logical region was not written (or is not finite)"
        assert nbad == 0, f"{nbad} elements outside the bound (worst {frac:.3g} x bound)"
        worst.append(frac)
    if engine == 16:
        assert int(status[0]) == 0, f"range status {int(status[0])} on an in-range problem"
    return form, max(worst)


def _cases16(epi, out, ncu):
    """Shapes that steer launch16s_tiled to each of its forms on a device of ncu CUs (gemm16s.hip launch16s_tiled)."""
    rag = epi in RAGGED_N
    nb = BIAS_OPTIONAL & {epi}
    pz = max(2, ncu // 8)                 # z slices that leave 8 persistent slots per slice (G = ncu * per_cu / nz)
    if epi == G.EPI_HEAD:
        return [
            lin(100, 96, 192),                                 # 64x32 KS2 + loader waves, direct
            lin(1000, 128, 160),                               # 128x128 staged (N % 64 == 0)
            lin(300, 96, 160, wscale=2.0 ** -10),              # 128x128 direct, weight scaled (acc_scale 2^-10)
            lin(128 * 9 + 1, 32, 128, nz=pz, shared=True, b_act=True),    # persistent grid, shared A
            lin(1, 32, 64),
            lin(70, 64, 96, nz=3),
        ]
    cs = [
        lin(300, 62 if rag else 64, 96),                                   # 256x64
        lin(200, 34 if rag else 36, 64, no_bias=bool(nb)),                 # 256x64, N % 32 != 0: direct epilogue
        lin(256 * 9 + 7, 32, 128, nz=pz, shared=True, b_act=True),         # 256x64 persistent, zA = 0, B in W_hi
        lin(150, 94 if rag else 96, 192, wscale=2.0 ** -10, no_bias=bool(nb)),   # 64x32 KS2, acc_scale != 1
        lin(64 * (ncu // 3) + 1, 96, 192),                                 # 128x32 KS2
        lin(300, 96, 160),                                                 # 128x32
        lin(1, 96, 64),                                                    # M = 1
        conv(2, 50, 32, 96, 4, stride=2, tap_pair=True),                   # 128x32: reflect, stride 2, tap pairs (k = 2 stride)
        conv(3, 40, 32, 96, 5, dil=2, pad_mode=0),                         # zero padding, dilation 2
        conv(2, 3, 32, 96, 7),                                             # reflect, T_in shorter than the pad (Tp > T_in)
        lin(128 * (ncu // 8) + 1, 256, 192),                               # 128x64 KS2
        lin(128 * (ncu // 8) + 1, 254 if rag else 256, 160),               # 128x64
        lin(128 * 39 + 1, 382 if rag else 384, 64),                        # 128x128
        lin(128 * (ncu // 3) + 1, 384, 64, nz=1),                          # 128x192
        lin(80, 96, 128, nz=3, b_act=True),                                # nz > 1, zA != 0
    ]
    # a second K source: K1 = 96 is an odd number of K tiles, so the switch falls inside a pair on the KS = 2 forms
    cs += [lin(100, 96, 192, K1=96), lin(64 * (ncu // 3) + 1, 96, 192, K1=96), lin(300, 96, 224, K1=160, apad=32)]
    return cs


def _cases32(epi):
    """Shapes for each form of gemm.hip launch_tiled (512 workgroup slots: its cost model does not read the CU count)."""
    if epi == G.EPI_HEAD:
        return [lin(300, 96, 96), lin(1, 32, 64), lin(70, 64, 96, nz=2), lin(200, 128, 64, no_bias=False)]
    nb = BIAS_OPTIONAL & {epi}
    return [
        lin(300, 30 if epi in RAGGED_N else 32, 96),               # 128x32
        lin(300, 32, 96, no_bias=bool(nb)),
        conv(2, 50, 32, 64, 4, stride=2),                          # 128x64: reflect, stride 2
        conv(3, 40, 32, 48, 3, dil=2, pad_mode=0),                 # zero padding, dilation 2
        conv(2, 3, 32, 64, 7),                                     # T_in shorter than the pad
        lin(1, 96, 64),
        lin(128 * 300, 96, 32),                                    # 128x96
        lin(128 * 300 - 5, 128, 32),                               # 128x128
        lin(200, 64, 64, nz=4, shared=True, b_act=True),
        lin(90, 100, 64, nz=2, b_act=True),
    ]


EXPECT16 = {"256x64", "64x32ks2p2", "128x32ks2p1", "128x32", "128x64ks2p1", "128x64", "128x128", "128x192"}
EXPECT16_HEAD = {"64x32ks2p2", "128x128"}
EXPECT32 = {"128x32", "128x64", "128x96", "128x128"}


@pytest.mark.parametrize("pair", G.PAIRS16, ids=lambda p: f"{G.EPI_NAMES[p[0]]}-{G.OUT_NAMES[p[1]]}")
def test_gemm16s_pair(pair):
    epi, out = pair
    ncu = _ncu()
    forms, staged, cache, grids, worst = set(), set(), set(), set(), 0.0
    for i, c in enumerate(_cases16(epi, out, ncu)):
        try:
            f, w = _run(16, epi, out, G.PRO_NONE, c, seed=1000 * epi + 10 * out + i)
        except AssertionError as e:
            raise AssertionError(f"case {i} {dict(c)}: {e}") from None
        forms.add(_form_name(f))
        staged.add(f.staged)
        cache.add(f.bias_cache)
        grids.add("persistent" if f.G < f.tiles else "one-shot")
        worst = max(worst, w)
    name = f"gemm16s {G.EPI_NAMES[epi]}/{G.OUT_NAMES[out]}"
    print(f"{name}: forms {sorted(forms)}, staged {sorted(staged)}, bias cache {sorted(cache)}, grids {sorted(grids)}, "
          f"worst error {worst:.3g} of the bound")
    parity_log.record(name, forms=sorted(forms), worst_of_bound=worst)
    assert forms == (EXPECT16_HEAD if epi == G.EPI_HEAD else EXPECT16), forms
    assert grids == {"persistent", "one-shot"}
    if pair in STAGEABLE16:
        assert staged == {0, 1}
    if epi in BIAS_OPTIONAL and epi != G.EPI_BIAS_GAMMA_RES:
        assert cache == {0, 1}


@pytest.mark.parametrize("pair", G.PAIRS32, ids=lambda p: f"{'ELU' if p[0] else 'NONE'}-{G.EPI_NAMES[p[1]]}")
def test_gemm_fp32_pair(pair):
    pro, epi = pair
    forms, worst = set(), 0.0
    for i, c in enumerate(_cases32(epi)):
        try:
            f, w = _run(32, epi, G.OUT_F32, pro, c, seed=500 * epi + 7 * pro + i)
        except AssertionError as e:
            raise AssertionError(f"case {i} {dict(c)}: {e}") from None
        forms.add(_form_name(f))
        worst = max(worst, w)
    name = f"gemm {'ELU' if pro else 'NONE'}/{G.EPI_NAMES[epi]}"
    print(f"{name}: forms {sorted(forms)}, worst error {worst:.3g} of the bound")
    parity_log.record(name, forms=sorted(forms), worst_of_bound=worst)
    assert forms == ({"128x128"} if epi == G.EPI_HEAD else EXPECT32), forms


def _range_status(engine, epi, out, pro, big):
    """Status word after a small problem whose single largest output is `big` (placed through the bias)."""
    from wavtokenizer_amd import _capi
    M, N, K = 64, 64, 64
    gen = torch.Generator().manual_seed(7)
    A = (torch.randn(M, K, generator=gen) * 0.01).cuda()
    B = (torch.randn(N, K, generator=gen) * 0.01).cuda()
    bias = torch.zeros(M if epi == G.EPI_BIAS_ROW else N)
    bias[5] = big
    bias = bias.cuda()
    R = torch.zeros(M, N).cuda()
    gamma = torch.ones(N).cuda()
    C = torch.zeros(M * N).cuda()
    C2 = torch.zeros(M * N).cuda()
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _capi.WtGemmDesc()
    d.size = ctypes.sizeof(d)
    d.engine, d.epi, d.out, d.pro = (0 if engine == 16 else 1), epi, out, pro
    d.M, d.N, d.K, d.nz, d.alpha = M, N, K, 1, 1.0
    d.T_in = d.T_out = M
    d.Cin, d.taps, d.stride, d.dil = K, 1, 1, 1
    d.a_rstride, d.w_rstride, d.c_rstride, d.r_rstride = K, K, N, N
    d.head_kb = N // 2
    d.A, d.B, d.bias, d.R, d.gamma, d.C, d.C2, d.status = (A.data_ptr(), B.data_ptr(), bias.data_ptr(), R.data_ptr(),
                                                          gamma.data_ptr(), C.data_ptr(), C2.data_ptr(), status.data_ptr())
    ws = torch.empty(max(_capi.lib.wt_gemm_probe_workspace_bytes(ctypes.byref(d)), 256), dtype=torch.uint8, device="cuda")
    assert _capi.lib.wt_gemm_probe(ctypes.byref(d), None, _ptr(ws), None) == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    return int(status[0]) & 2


@pytest.mark.parametrize("engine,pair", [(16, p) for p in G.PAIRS16] + [(32, p) for p in G.PAIRS32])
def test_range_report(engine, pair):
    """An S32 output of magnitude 70000 sets WT_STATUS_RANGE, one of 60000 leaves it clear.  OUT_F32_AND_S32 reports
    through its S32 copy in C2; OUT_S32_DUAL_ELU reports a large negative v through C although C2 = elu(v) is about -1.
    fp32-only outputs (and gemm.hip) never set it; the head's outputs are clipped at 100 and cannot reach it."""
    epi, out = pair if engine == 16 else (pair[1], G.OUT_F32)
    pro = pair[0] if engine == 32 else G.PRO_NONE
    big = -70000.0 if out == G.OUT_S32_DUAL_ELU else 70000.0
    s32_out = engine == 16 and out != G.OUT_F32 and epi != G.EPI_HEAD
    assert _range_status(engine, epi, out, pro, big) == (2 if s32_out else 0)
    assert _range_status(engine, epi, out, pro, big * 6 / 7) == 0
