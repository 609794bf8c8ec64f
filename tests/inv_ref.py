"""Helpers of tests/test_batch_invariance.py: a block of rows (or one clip) with fixed contents is run alone and again inside
larger problems that differ only in batch extent; its output must be the same words.  This module holds the placement of the
block among filler rows, the extraction of its output rows, the word-for-word comparison, a mirror of the GEMM launchers' tile
choice (to size the extents for each form on any CU count) and lean probe runners that keep the operands on the device.
Nothing here computes a reference value: the solo run is the reference, and the only comparison is integer equality."""
import ctypes
import math

import numpy as np
import torch

from tests import gemm_ref as G

BLOCK = 70                       # rows of the block: no multiple of 16, and it spans a 64-row tile edge
NAN32 = 0x7FC00000
SBK = 32                         # K tile of both GEMM engines


def ncu():
    from wavtokenizer_amd import _capi
    cu = ctypes.c_int32()
    assert _capi.lib.wt_device_info(torch.cuda.current_device(), ctypes.byref(cu), None, None) == 0
    return cu.value


def r_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ comparison
def _ordered(bits):
    """int32 fp32 bit patterns -> integers whose difference is the distance in ulps (sign-magnitude to two's complement)."""
    b = bits.astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def diff_words(got, want, s32=False):
    """(number of differing words, largest ulp distance among fp32 words or None) of two integer views of the same shape."""
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, w.shape, g.dtype, w.dtype)
    bad = g != w
    n = int(bad.sum())
    if n == 0 or s32 or g.dtype != np.int32:
        return n, None
    return n, int(np.abs(_ordered(g[bad]) - _ordered(w[bad])).max())


def words(t, s32=False):
    """A device or host tensor of 32-bit slots -> numpy integers: int32 words, or for S32 data the int16 halves (hi and lo)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.int64:
        return t.numpy()
    t = t.view(torch.int32)
    return (t.view(torch.int16) if s32 else t).numpy()


def assert_same_words(got, want, what, s32=False):
    """Raw integer equality: NaN payloads and the sign of zero count."""
    n, ulp = diff_words(got, want, s32)
    assert n == 0, f"{what}: {n} of {np.asarray(got).size} words differ from the solo run" + (f" (up to {ulp} ulp)" if ulp is not None else "")


def assert_written(t, what):
    """No 32-bit slot of a solo output still holds the NaN it was pre-filled with: two unwritten outputs would compare equal."""
    w = words(t)
    assert not bool((w == NAN32).any()), f"{what}: {int((w == NAN32).sum())} output words were never written"


def positions(M, block=BLOCK):
    """Offsets of the block in a problem of M rows: 0, one that is no multiple of 16 inside a later tile (128 k + 37), and
    flush with the end; fewer where they would overlap."""
    if M == block:
        return [0]
    out = [0]
    k = max(1, (M // 2) // 128)
    mid = 128 * k + 37
    if mid >= block and mid + block <= M - block:
        out.append(mid)
    if M - block >= block:
        out.append(M - block)
    assert len(out) >= 2 or M < 2 * block, (M, out)
    return out


def embed(filler, block, offs, dim=0):
    """A copy of `filler` with `block` written at each offset of `offs` along `dim`."""
    out = filler.clone()
    n = block.shape[dim]
    for o in offs:
        out.narrow(dim, o, n).copy_(block)
    return out


# ------------------------------------------------------------------------------------------------ the launchers' tile choice
def form_name(f):
    return f"{f.BM}x{f.BN}" + (f"ks2p{f.prod}" if f.ks == 2 else "")


def form16(M, N, K, nz, cus, head=False, taps=1, a2=False):
    """The form gemm16s.hip launch16s_tiled picks (no environment switches)."""
    nkt = K // SBK
    ks2 = nkt % 2 == 0 and nkt >= 6
    c = lambda a, b: -(-a // b)
    if head:
        return "64x32ks2p2" if ks2 and c(M, 64) * c(N, 32) * nz <= cus else "128x128"
    if N <= 64:
        return "256x64"
    t128 = c(M, 128) * c(N, 128) * nz
    cols32 = c(N, 32) * nz
    t32, t64 = c(M, 128) * cols32, c(M, 64) * cols32
    if ks2 and t64 <= cus:
        return "64x32ks2p2"
    if ks2 and t32 <= cus and nz == 1:
        return "128x32ks2p1"
    if t128 <= 32:
        return "128x32"
    if t128 <= 100:
        return "128x64ks2p1" if ks2 and nz == 1 and taps <= 7 and not a2 else "128x64"
    tm = c(M, 128)
    cost = lambda bn, eff: math.ceil(tm * c(N, bn) * nz / cus) * bn / eff
    return "128x128" if cost(128, 0.82) < cost(192, 1.0) else "128x192"


def form32(M, N, nz=1):
    """The form gemm.hip launch_tiled picks (512 workgroup slots: it does not read the CU count)."""
    c = lambda a, b: -(-a // b)
    if N <= 32:
        return "128x32"
    if N <= 64:
        return "128x64"
    tm = c(M, 128)
    cost = lambda bn, eff: math.ceil(tm * c(N, bn) * nz / 512.0) * bn / eff
    c128, c96, c64 = cost(128, 1.0), cost(96, 0.97), cost(64, 0.88)
    if c64 < c96 and c64 < c128:
        return "128x64"
    return "128x96" if c96 < c128 else "128x128"


def extent_for(pick, want, first, limit=40000):
    """The extent (rows, or clips) at which pick(extent) == want: `first` (the value worked out for 256 CUs) if the rule agrees on
    this device, else the smallest 128 k + 1 that does."""
    if pick(first) == want:
        return first
    for k in range(1, limit // 128):
        if pick(128 * k + 1) == want:
            return 128 * k + 1
    raise AssertionError(f"no extent up to {limit} selects {want}")


# ------------------------------------------------------------------------------------------------ GEMM probe, operands on the device
RES_EPIS = (G.EPI_BIAS_RES, G.EPI_BIAS_RES_ELU, G.EPI_BIAS_GAMMA_RES)
FMTS = {G.OUT_F32: ["f32"], G.OUT_S32: ["s32"], G.OUT_S32_DUAL_ELU: ["s32", "s32"], G.OUT_F32_AND_S32: ["f32", "s32"]}
ALPHA = 0.0883883


class LinFamily:
    """One linear problem family: N, K and everything indexed by column fixed (weight of nz slices with its per-tensor scale,
    bias, gamma), row-indexed operands (A, the second K source, R, the EPI_BIAS_ROW bias) drawn ONCE at the largest extent
    and sliced (a shorter randn is not a prefix of a longer one), and the block's own rows, which travel with it."""

    def __init__(self, N, K, M_max, nz_max, seed, head=False, shared=False):
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen)
        self.N, self.K, self.M_max, self.nz_max, self.head, self.shared = N, K, M_max, nz_max, head, shared
        self.r_pitch = r_up(N, 4) + 32
        if head:
            kb = N // 2
            W = torch.stack([G.pack_head_rows(rnd(kb, K) / K ** 0.5, rnd(kb, K) / K ** 0.5 * 2) for _z in range(nz_max)])
            bias = G.pack_head_rows(rnd(kb) * 2 + 2, rnd(kb))
        else:
            W = rnd(nz_max, N, K) / K ** 0.5
            bias = rnd(N)
        self.W = W.float().contiguous().cuda()
        self.bias = bias.float().contiguous().cuda()
        self.gamma = (torch.rand(N, generator=gen) + 0.25).float().cuda()
        self.block = dict(A=rnd(BLOCK, K).float().cuda(), R=rnd(BLOCK, self.r_pitch).float().cuda(), rowbias=rnd(BLOCK).float().cuda())
        na = 1 if shared else nz_max
        self.fill = dict(A=rnd(na, M_max, K).float().cuda(), R=rnd(M_max, self.r_pitch).float().cuda(), rowbias=rnd(M_max).float().cuda())

    def run(self, engine, epi, out, M, nz=1, offs=(0,), K1=None, b_act=False, pro=G.PRO_NONE):
        """One probe launch of M rows and nz slices with the block at every offset of `offs` in slice 0.
        Returns (form, [per offset: [per output: integer words of the block's rows, the pad columns of the pitch included]])."""
        from wavtokenizer_amd import _capi
        N, K = self.N, self.K
        assert M <= self.M_max and nz <= self.nz_max
        na = 1 if self.shared else nz
        A = self.fill["A"][:na, :M].clone()
        for o in offs:
            A[0, o:o + BLOCK] = self.block["A"]
        d = _capi.WtGemmDesc()
        d.size = ctypes.sizeof(d)
        d.engine, d.epi, d.out, d.pro = engine, epi, out, pro
        d.b_is_act = 1 if b_act else 0
        d.M, d.N, d.K, d.nz, d.alpha = M, N, K, nz, ALPHA
        d.stride, d.dil, d.taps = 1, 1, 1
        d.T_in = d.T_out = M
        d.Cin = K
        keep = [A]
        if K1:
            assert na == 1
            A1, A2 = A[0, :, :K1].contiguous(), A[0, :, K1:].contiguous()
            keep += [A1, A2]
            d.A, d.A2, d.K1, d.a2_rstride, d.a_rstride = A1.data_ptr(), A2.data_ptr(), K1, K - K1, K1
            d.zA = 0
        else:
            d.A, d.a_rstride = A.data_ptr(), K
            d.zA = 0 if self.shared else M * K
        d.B, d.w_rstride, d.zW = self.W.data_ptr(), K, N * K
        if epi == G.EPI_BIAS_ROW:
            rb = embed(self.fill["rowbias"][:M], self.block["rowbias"], offs)
            keep.append(rb)
            d.bias = rb.data_ptr()
        elif epi != G.EPI_SCALE:
            d.bias = self.bias.data_ptr()
        if epi in RES_EPIS:
            R = embed(self.fill["R"][:M], self.block["R"], offs)
            keep.append(R)
            d.R, d.r_rstride = R.data_ptr(), self.r_pitch
        if epi == G.EPI_BIAS_GAMMA_RES:
            d.gamma = self.gamma.data_ptr()
        if self.head:
            d.head_kb = N // 2
        return _launch_gemm(d, out, M, N, nz, [(o, BLOCK) for o in offs], keep)


class ConvFamily:
    """A conv gather problem (time-major activations [clips][T_in][Cin]); the block is one clip, with the rows of R and of
    the EPI_BIAS_ROW bias that belong to its output frames."""

    def __init__(self, case_of, clips_max, seed):
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen)
        self.case_of = case_of
        c = case_of(1)
        self.N, self.K, self.T_out = c.N, c.K, c.T_out
        self.r_pitch = r_up(c.N, 4) + 32
        w = (rnd(c.N, c.Cin, c.k) / (c.Cin * c.k) ** 0.5).float()
        order = G.tap_order(c.k, c.stride, c.tap_pair)
        self.W = w[:, :, order].permute(0, 2, 1).reshape(c.N, c.K).contiguous().cuda()
        self.bias = rnd(c.N).float().cuda()
        self.gamma = (torch.rand(c.N, generator=gen) + 0.25).float().cuda()
        self.block = dict(A=rnd(c.T_in, c.Cin).float().cuda(), R=rnd(c.T_out, self.r_pitch).float().cuda(), rowbias=rnd(c.T_out).float().cuda())
        self.fill = dict(A=rnd(clips_max, c.T_in, c.Cin).float().cuda(), R=rnd(clips_max * c.T_out, self.r_pitch).float().cuda(),
                         rowbias=rnd(clips_max * c.T_out).float().cuda())

    def run(self, engine, epi, out, clips, slots=(0,)):
        from wavtokenizer_amd import _capi
        c = self.case_of(clips)
        M, N, K, To = c.M, c.N, c.K, c.T_out
        A = embed(self.fill["A"][:clips], self.block["A"][None], slots)
        d = _capi.WtGemmDesc()
        d.size = ctypes.sizeof(d)
        d.engine, d.epi, d.out, d.pro = engine, epi, out, G.PRO_NONE
        d.M, d.N, d.K, d.nz, d.alpha = M, N, K, 1, ALPHA
        d.T_in, d.T_out, d.Cin, d.taps, d.stride, d.dil = c.T_in, c.T_out, c.Cin, c.k, c.stride, c.dil
        d.pad_left, d.pad_mode, d.tap_pair = c.pl, c.pad_mode, 1 if c.tap_pair else 0
        d.Tp = max(c.T_in, max(c.pl, c.pr) + 1) if c.pad_mode == 1 else c.T_in
        d.a_bstride, d.a_rstride, d.w_rstride = c.T_in * c.Cin, c.Cin, K
        d.A, d.B = A.data_ptr(), self.W.data_ptr()
        keep = [A]
        offs = [s * To for s in slots]
        if epi == G.EPI_BIAS_ROW:
            rb = embed(self.fill["rowbias"][:M], self.block["rowbias"], offs)
            keep.append(rb)
            d.bias = rb.data_ptr()
        elif epi != G.EPI_SCALE:
            d.bias = self.bias.data_ptr()
        if epi in RES_EPIS:
            R = embed(self.fill["R"][:M], self.block["R"], offs)
            keep.append(R)
            d.R, d.r_rstride = R.data_ptr(), self.r_pitch
        if epi == G.EPI_BIAS_GAMMA_RES:
            d.gamma = self.gamma.data_ptr()
        return _launch_gemm(d, out, M, N, 1, [(o, To) for o in offs], keep)


def _launch_gemm(d, out, M, N, nz, spans, keep):
    from wavtokenizer_amd import _capi
    pitch = r_up(N, 32) + 32
    zC = (M + 2) * pitch + 32
    d.c_rstride, d.zC = pitch, zC
    fmts = FMTS[out]
    bufs = [torch.full((nz * zC,), NAN32, dtype=torch.int32, device="cuda") for _f in fmts]
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    d.C = bufs[0].data_ptr()
    d.C2 = bufs[1].data_ptr() if len(bufs) > 1 else None
    d.status = status.data_ptr()
    nws = _capi.lib.wt_gemm_probe_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device="cuda")
    form = _capi.WtLaunchForm()
    rc = _capi.lib.wt_gemm_probe(ctypes.byref(d), ctypes.byref(form), ctypes.c_void_p(ws.data_ptr()), None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    assert int(status[0]) == 0, f"range status {int(status[0])} on an in-range problem"
    del keep
    res = []
    for o, n in spans:           # slice 0
        rows = [b[:M * pitch].reshape(M, pitch)[o:o + n] for b in bufs]
        for b in rows:
            assert_written(b[:, :N // 32 * 32], "the block's rows")      # (whole 32-slot groups: S32 keeps hi and lo halves 32 apart)
        res.append([words(b, s32=(f == "s32")) for f, b in zip(fmts, rows)])
    return form, res


def compare_blocks(solo, got, out, what):
    """Every placement's outputs (both arrays of the dual formats) against the solo run's."""
    for i, blk in enumerate(got):
        for f, g, w in zip(FMTS[out], blk, solo):
            assert_same_words(g, w, f"{what}, placement {i}, {f} output", s32=(f == "s32"))


# ------------------------------------------------------------------------------------------------ wt_op_probe
def op_probe(op, **kw):
    """One wt_op_probe call -> the form's name, as tests/test_decoder_ops.py spells it (that file's own coverage set is not
    touched from here)."""
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
    if k in ("dwconv_ln", "rownorm"):
        return f"{k}<{f.variant},{f.variant2}>"
    if k == "softmax_reg":
        return f"{k}<{f.variant}>"
    return k


def nan_out(n):
    """n fp32 output slots on the device, pre-filled with NaN."""
    return torch.full((n,), NAN32, dtype=torch.int32, device="cuda")
