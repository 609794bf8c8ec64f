"""Float64 references and the per-element error bound for the GEMM epilogues (tests/test_gemm_epilogues.py,
tests/test_gemm_checks.py).  Everything here is built from the definitions (common.h Epi / Out16s, heads.py:55-59,
the nn.Linear / Conv1d layouts), never from a kernel output.  CPU only."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# common.h
PRO_NONE, PRO_ELU = 0, 1
EPI_BIAS, EPI_BIAS_RES, EPI_BIAS_GELU, EPI_BIAS_GAMMA_RES, EPI_HEAD = 0, 1, 2, 3, 4
EPI_SCALE, EPI_BIAS_ROW, EPI_BIAS_RES_ELU, EPI_BIAS_ELU = 7, 8, 9, 10
OUT_F32, OUT_S32, OUT_S32_DUAL_ELU, OUT_F32_AND_S32 = 0, 1, 2, 3
EPI_NAMES = {0: "BIAS", 1: "BIAS_RES", 2: "BIAS_GELU", 3: "BIAS_GAMMA_RES", 4: "HEAD", 7: "SCALE", 8: "BIAS_ROW",
             9: "BIAS_RES_ELU", 10: "BIAS_ELU"}
OUT_NAMES = {0: "F32", 1: "S32", 2: "S32_DUAL_ELU", 3: "F32_AND_S32"}

# The pairs the launchers instantiate (gemm16s.hip WT_GEMM16S_PAIRS, gemm.hip WT_GEMM_PAIRS) minus the argmax epilogue,
# which has its own reference and tests (tests/vq_ref.py, tests/test_vq_ops.py): gemm16s (epi, out), gemm (pro, epi)
PAIRS16 = [(EPI_BIAS, OUT_F32), (EPI_BIAS, OUT_S32), (EPI_BIAS, OUT_S32_DUAL_ELU), (EPI_BIAS, OUT_F32_AND_S32),
           (EPI_BIAS_RES, OUT_F32), (EPI_BIAS_ELU, OUT_S32), (EPI_BIAS_RES_ELU, OUT_S32), (EPI_BIAS_GELU, OUT_S32),
           (EPI_BIAS_GAMMA_RES, OUT_F32), (EPI_HEAD, OUT_S32), (EPI_SCALE, OUT_F32), (EPI_BIAS_ROW, OUT_S32)]
PAIRS32 = [(PRO_NONE, EPI_BIAS), (PRO_ELU, EPI_BIAS), (PRO_ELU, EPI_BIAS_RES), (PRO_ELU, EPI_BIAS_RES_ELU),
           (PRO_NONE, EPI_BIAS_RES), (PRO_NONE, EPI_BIAS_GELU), (PRO_NONE, EPI_BIAS_GAMMA_RES), (PRO_NONE, EPI_HEAD),
           (PRO_NONE, EPI_SCALE), (PRO_NONE, EPI_BIAS_ROW)]

# Error bound.  A product of split-f16 operands (x = hi + lo 2^-11, three f16 MFMAs, lo.lo dropped) is within 2^-22 of the
# exact one relative to |a w|, an fp32 product is exact; the fp32 accumulation over K <= 2304 adds at most
# (K / 32 + 5) 2^-24 <= 77 2^-24 ~ 19 2^-22 relative to sum |a w|.  TOL = 64 2^-22 (~1.5e-5) leaves a margin of about 3
# over that worst case; the measured errors sit far below it (the tests print the worst fraction of the bound).
TOL = 64 * 2.0 ** -22
ULP = 2.0 ** -23              # one fp32 rounding (with margin) of an epilogue operation, relative to its result
S32_ENC = 2.0 ** -22          # hi + lo 2^-11 carries 22 significant bits
ABS_FLOOR = 2.0 ** -34        # the f16 subnormal floor of the lo half
FN_ABS = 1e-6                 # the epilogues' ELU / GELU approximations (< 4e-7 absolute, gemm16s.hip) with margin
GELU_LIP = 1.13               # max |gelu'(x)|


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def elu(x):
    return torch.where(x > 0, x, torch.expm1(x))


def epilogue(epi, out, acc, mag, bias=None, R=None, gamma=None, alpha=1.0, head_kb=0):
    """(outputs, bounds): the float64 result of the epilogue on acc [.., M, N] (= sum_k a_k w_k) and its per-element
    bound, from mag = sum_k |a_k w_k| (+ the operand-format terms the caller adds).  outputs is a list: [C] or [C, C2];
    bias is [N] (BIAS_ROW: [M]), R [M][N], gamma [N]."""
    e_acc = TOL * mag + ABS_FLOOR
    if epi == EPI_SCALE:
        v = alpha * acc
        e = abs(alpha) * e_acc + ULP * v.abs()
        outs, bounds = [v], [e]
    elif epi == EPI_HEAD:
        kb = head_kb
        bb = torch.zeros(acc.shape[-1], dtype=acc.dtype) if bias is None else bias
        lm_c, ph_c = unpack_head(acc + bb, kb)
        lm_e, ph_e = unpack_head(e_acc + ULP * (acc + bb).abs(), kb)
        m = torch.clamp(torch.exp(lm_c), max=100.0)
        re, im = m * torch.cos(ph_c), m * torch.sin(ph_c)
        # d(min(e^l, 100) (cos, sin)(p)) <= m (|dl| + |dp|); exp / sincos / the products: a few ulp of m
        e = m * (lm_e + ph_e) + 8 * ULP * m
        outs, bounds = [torch.cat([re, im], -1)], [torch.cat([e, e], -1)]
    else:
        if epi == EPI_BIAS_ROW:
            v = acc if bias is None else acc + bias[..., :, None]
        else:
            v = acc if bias is None else acc + bias
        e_v = e_acc + ULP * v.abs()
        if epi == EPI_BIAS:
            outs, bounds = [v], [e_v]
        elif epi == EPI_BIAS_ROW:
            outs, bounds = [v], [e_v]
        elif epi == EPI_BIAS_RES:
            y = v + R
            outs, bounds = [y], [e_v + ULP * y.abs()]
        elif epi == EPI_BIAS_RES_ELU:
            u = v + R
            y = elu(u)
            outs, bounds = [y], [e_v + ULP * u.abs() + FN_ABS + ULP * y.abs()]
        elif epi == EPI_BIAS_ELU:
            y = elu(v)
            outs, bounds = [y], [e_v + FN_ABS + ULP * y.abs()]
        elif epi == EPI_BIAS_GELU:
            y = gelu(v)
            outs, bounds = [y], [GELU_LIP * e_v + FN_ABS + ULP * y.abs()]
        elif epi == EPI_BIAS_GAMMA_RES:
            y = R + gamma * v
            outs, bounds = [y], [gamma.abs() * e_v + ULP * ((gamma * v).abs() + y.abs())]
        else:
            raise ValueError(epi)
        if out == OUT_S32_DUAL_ELU:
            y2 = elu(outs[0])
            outs.append(y2)
            bounds.append(bounds[0] + FN_ABS + ULP * y2.abs())
        elif out == OUT_F32_AND_S32:
            outs.append(outs[0])
            bounds.append(bounds[0])
    # the S32 encoding of an S32 output
    s32 = {OUT_F32: [False], OUT_S32: [True], OUT_S32_DUAL_ELU: [True, True], OUT_F32_AND_S32: [False, True]}[out]
    bounds = [b + (S32_ENC * o.abs() if s else 0) for o, b, s in zip(outs, bounds, s32)]
    return outs, bounds


def pack_head_rows(lm_rows, ph_rows):
    """The head's 32-row groups (weights.cpp head packing): 16 log-magnitude rows, then the 16 phase rows of the same
    spectrum slots.  lm_rows, ph_rows [kb][...] -> [2 kb][...]"""
    kb = lm_rows.shape[0]
    assert kb % 16 == 0
    out = torch.empty((2 * kb,) + tuple(lm_rows.shape[1:]), dtype=lm_rows.dtype)
    for s in range(kb):
        pm = (s // 16) * 32 + s % 16
        out[pm] = lm_rows[s]
        out[pm + 16] = ph_rows[s]
    return out


def unpack_head(packed, kb):
    """Inverse of pack_head_rows along the last axis: [..., 2 kb] -> ([..., kb] log-magnitude, [..., kb] phase)."""
    s = torch.arange(kb)
    pm = (s // 16) * 32 + s % 16
    return packed[..., pm], packed[..., pm + 16]


def tap_order(k, stride, tap_pair):
    """Tap held by K slot q (common.h GemmArgs::tap_pair: q -> (q >> 1) + (q & 1) * stride for k = 2 * stride)."""
    return [(q >> 1) + (q & 1) * stride for q in range(k)] if tap_pair else list(range(k))


def conv_ref(x, w, stride, dil, pl, pr, pad_mode, T_out, pro=PRO_NONE):
    """x [clips][Cin][T] float64, w [N][Cin][k] -> (acc, mag) [clips][T_out][N] time-major, through F.conv1d and the
    oracle's padding (pad1d_reflect: encoder/modules/conv.py:79-96, short inputs included)."""
    from oracle.cpu_ref import pad1d_reflect
    if pro == PRO_ELU:
        x = elu(x)
    pad = (lambda t: pad1d_reflect(t, (pl, pr))) if pad_mode == 1 else (lambda t: F.pad(t, (pl, pr)))
    acc = F.conv1d(pad(x), w, stride=stride, dilation=dil)[..., :T_out]
    mag = F.conv1d(pad(x.abs()), w.abs(), stride=stride, dilation=dil)[..., :T_out]
    assert acc.shape[-1] == T_out
    return acc.transpose(1, 2), mag.transpose(1, 2)


def check(got, ref, bound):
    """(n_bad, worst |got - ref| / bound, all finite) over every logical element."""
    got = torch.as_tensor(got, dtype=torch.float64)
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs() / bound
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return int((err > 1.0).sum()), float(err.max()) if err.numel() else 0.0, finite


def decode_s32_rows(h16, rows, cols):
    """S32 rows (int16 view of [rows][pitch] fp32 slots, pitch % 32 == 0) -> float64 [rows][cols]:
    every 32 values of a row are 128 bytes [32 x f16 hi | 32 x f16 lo], value = hi + lo / 2048."""
    h = h16.view(torch.float16).reshape(rows, -1, 2, 32).double()
    v = (h[:, :, 0, :] + h[:, :, 1, :] / 2048.0).reshape(rows, -1)
    return v[:, :cols]


def s32_logical_mask(rows, pitch, cols):
    """bool [rows][2 pitch] over the int16 halves of S32 rows: True where a half (hi or lo) of a column < cols lies."""
    e = np.arange(cols)
    pos = (e // 32) * 64 + e % 32
    m = np.zeros((rows, 2 * pitch), bool)
    m[:, pos] = True
    m[:, pos + 32] = True
    return m
