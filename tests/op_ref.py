"""Float64 references and per-element error bounds for the non-GEMM kernels of csrc/ops.hip (tests/test_decoder_ops.py on
the GPU, tests/test_op_checks.py on the CPU).  Everything is written from the definitions the kernel comments cite
(GroupNorm(32, C, eps) with biased variance, LayerNorm, depthwise conv k 7 p 3, AdaLayerNorm scale / shift, softmax,
x sigmoid(x), reflect-padded conv, ConvTranspose1d with its trim, the ISTFT tail), never from a kernel output.  CPU only.

Every reference returns (ref, bound).  The bounds are propagated through the formula, one fp32 rounding (gemm_ref.ULP =
2^-23, i.e. twice the unit roundoff u = 2^-24, so "k ULP" below covers 2 k roundings) per operation:

  sums      A sum of n terms accumulated as per-lane partial sums followed by a wave reduction passes every term through
            at most `depth` additions; its error is at most depth u sum|term| = depth / 2 ULP sum|term|.
            sum_k(n) = (ceil(n / 256) + 12) / 2 assumes at least 256-way partial sums of 4-element steps (GroupNorm:
            gn_stats_kernel strides 256 threads over the group; the slab kernels have fewer, shorter chains), 6 shuffle
            levels, the join of up to 4 waves, the 1 / n scaling and, for the chunked form, 3 roundings per merged chunk at
            <= 11 chunks.  dot_k(depth) = depth / 2 for the short convolutions, whose chain lengths are written at the call.
  exp       v_exp_f32 and v_rcp_f32 are specified to 1 ulp (AMD CDNA3 / CDNA4 instruction set reference, "V_EXP_F32",
            "V_RCP_F32"); __expf(x) = v_exp_f32(x log2 e) rounds its argument once more, an absolute error u |x| log2 e
            in the exponent, i.e. a relative error |x| u in the result: exp_rel(x) = (2 + |x|) ULP covers both (and
            expf / expm1f of the device library, which are within 1 ulp).  The ELU built on it is within FN_ABS
            (gemm_ref: (2 + |x|) e^x ULP <= 2 ULP for x <= 0, plus the rounding of e - 1).
  floors    results below the smallest normal fp32 number 2^-126 may be flushed to zero.
"""
import math

import torch
import torch.nn.functional as F

from tests import gemm_ref as G

ULP = G.ULP
TINY = 2.0 ** -126
SWISH_LIP = 1.1           # max |d/dx x sigmoid(x)| = 1.0998


def sum_k(n):
    return (math.ceil(n / 256) + 12) / 2


def dot_k(depth):
    return depth / 2


def exp_rel(x):
    return (2 + x.abs()) * ULP


def s32(y, e):
    """Bound of an S32-encoded output (hi + lo 2^-11: 22 significant bits, f16 subnormal floor of the lo half)."""
    return e + G.S32_ENC * y.abs() + G.ABS_FLOOR


def swish(v, e_v):
    """v sigmoid(v) evaluated as v * rcp(1 + exp(-v)) on an argument known to e_v."""
    y = v * torch.sigmoid(v)
    sneg = torch.sigmoid(-v)                    # e^-v / (1 + e^-v): the weight of exp's relative error in 1 + e^-v
    # exp, the add, the reciprocal, the product; where e^-v overflows (v < -88.7) sigmoid is below 2^-126 and reads as 0
    e = SWISH_LIP * e_v + y.abs() * (exp_rel(v) * sneg + 3 * ULP) + v.abs() * TINY * 4
    return y, e


def elu(x):
    return G.elu(x)


# ------------------------------------------------------------------------------------------------ normalisations
def _norm_terms(v, dims, eps, k_sum, e_in):
    """mean, var (biased), rstd of v over dims with the error of the fp32 two-pass (or chunk-merged) evaluation:
    (mean, rstd, e_mean, rel_rstd).  e_in: per-element error of v itself (None: exact inputs)."""
    mean = v.mean(dims, keepdim=True)
    var = ((v - mean) ** 2).mean(dims, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    e_mean = k_sum * ULP * v.abs().mean(dims, keepdim=True)
    spread = e_mean
    if e_in is not None:
        e_mean = e_mean + e_in.mean(dims, keepdim=True)
        spread = e_mean + torch.sqrt((e_in ** 2).mean(dims, keepdim=True))
    # sum (v - m^)^2 / n: the squares and their sum are relative ((k_sum + 4) ULP); a mean off by delta adds delta^2, and
    # partial statistics taken about differently-rounded means (Chan's merge) or perturbed inputs add a cross term
    # <= 2 sqrt(var) delta
    d_var = (k_sum + 4) * ULP * var + 2 * torch.sqrt(var) * spread + spread ** 2 + TINY
    rel_rstd = 0.5 * d_var / (var + eps) + 4 * ULP          # sqrt and the division, 2 ULP each
    return mean, rstd, e_mean, rel_rstd


def groupnorm(x, gamma, beta, groups, eps=1e-6, act=False, out_s32=False):
    """GroupNorm(groups, C, eps, affine) on time-major x [B][L][C] as the kernels evaluate it:
    scale = rstd gamma, shift = beta - mean scale, y = x scale + shift (then x sigmoid(x)).
    Returns {"y": (ref, bound), "scale": (ref, bound), "shift": (ref, bound)}, scale / shift [B][C]."""
    B, L, C = x.shape
    cg = C // groups
    xg = x.reshape(B, L, groups, cg)
    mean, rstd, e_mean, rel_rstd = _norm_terms(xg, (1, 3), eps, sum_k(L * cg), None)
    g, b = gamma.reshape(1, 1, groups, cg), beta.reshape(1, 1, groups, cg)
    sc = rstd * g
    rel_sc = rel_rstd + ULP
    sh = b - mean * sc
    y = (xg - mean) * sc + b
    e_sc = sc.abs() * rel_sc
    e_sh = mean.abs() * sc.abs() * (rel_sc + ULP) + e_mean * sc.abs() + ULP * sh.abs()
    # the scale error acts on x - mean (x scale and mean scale carry the same scale); the products x scale and mean scale
    # are rounded relative to themselves: the term in (|x| + |mean|) rstd |gamma| that a large mean stresses
    e_y = ((xg - mean).abs() * sc.abs() * rel_sc + e_mean * sc.abs()
           + ULP * ((xg.abs() + mean.abs()) * sc.abs() + sh.abs() + y.abs()))
    if act:
        y, e_y = swish(y, e_y)
    y, e_y = y.reshape(B, L, C), e_y.reshape(B, L, C)
    if out_s32:
        e_y = s32(y, e_y)
    return {"y": (y, e_y), "scale": (sc.expand(B, 1, groups, cg).reshape(B, C), e_sc.expand(B, 1, groups, cg).reshape(B, C)),
            "shift": (sh.expand(B, 1, groups, cg).reshape(B, C), e_sh.expand(B, 1, groups, cg).reshape(B, C))}


def dwconv(x, w, b):
    """Depthwise conv k 7 p 3 (zero padding) on time-major x [B][L][C], w [7][C]: (v, e_v); a serial chain of 7
    multiply-adds on the bias: depth 8."""
    B, L, C = x.shape
    xp = F.pad(x, (0, 0, 3, 3))
    v = b.expand(B, L, C).clone()
    mag = b.abs().expand(B, L, C).clone()
    for j in range(7):
        v = v + xp[:, j:j + L] * w[j]
        mag = mag + (xp[:, j:j + L] * w[j]).abs()
    return v, dot_k(8) * ULP * mag


def rownorm(mode, x, out_scale, out_shift, eps=1e-6, dw_w=None, dw_b=None, in_scale=None, in_shift=None, out_s32=False):
    """LayerNorm over C of every frame row of x [B][L][C], then * out_scale + out_shift.  mode 0: of the depthwise conv
    of x; 1: of x; 2: of x in_scale[b] + in_shift[b].  (y, bound)."""
    C = x.shape[-1]
    if mode == 0:
        v, e_in = dwconv(x, dw_w, dw_b)
    elif mode == 2:
        v = x * in_scale[:, None, :] + in_shift[:, None, :]
        e_in = ULP * ((x * in_scale[:, None, :]).abs() + v.abs())
    else:
        v, e_in = x, None
    mean, rstd, e_mean, rel_rstd = _norm_terms(v, (2,), eps, sum_k(C), e_in)
    t = (v - mean) * rstd
    y = t * out_scale + out_shift
    e = ((v - mean).abs() * rstd * (rel_rstd + 3 * ULP) + (e_mean + (e_in if e_in is not None else 0)) * rstd) * out_scale.abs()
    e = e + ULP * ((t * out_scale).abs() + y.abs())
    return y, (s32(y, e) if out_s32 else e)


# ------------------------------------------------------------------------------------------------------ softmax
def softmax(s, out_s32=False):
    """Softmax over the last axis of s [rows][L] as max / exp(s - max) / sum / divide: (p, bound).  The sum over L <= 2080
    columns: per-lane chains of ceil(L / 64) terms and 6 shuffle levels."""
    L = s.shape[-1]
    mx = s.max(-1, keepdim=True).values
    d = s - mx
    p = torch.softmax(s, -1)
    r = ULP * d.abs() + exp_rel(d)                         # rounding of s - max, then exp
    r_sum = (p * r).sum(-1, keepdim=True) + dot_k(math.ceil(L / 64) + 6) * ULP
    e = p * (r + r_sum + ULP) + TINY
    return p, (s32(p, e) if out_s32 else e)


# ----------------------------------------------------------------------------------------------------- ISTFT tail
def istft_tail(parts, win, n_fft, hop, center, dtype=torch.float64, reverse=False):
    """ISTFT after the four quarter transforms parts [4][B][L][Kq] = Ce, Co, Se, So [frame][0 .. N/4]:
    C[m] = Ce[m] + Co[m], C[N/2 - m] = Ce[m] - Co[m]; S[m] = Se[m] + So[m], S[N/2 - m] = So[m] - Se[m]  (m <= N/4)
    x[n] = C[n] - S[n], x[N - n] = C[n] + S[n]  (n <= N/2); windowed, overlap-added at the hop, divided by the
    overlap-added squared window and trimmed by (N - hop) / 2 ("same") or N / 2 ("center") at both ends.  (y, bound).
    dtype / reverse: the same formula in another precision, frames added in descending order (tests/test_op_checks.py)."""
    N, Q, Nh = n_fft, n_fft // 4, n_fft // 2
    Ce, Co, Se, So = (parts[i][..., :Q + 1] for i in range(4))
    B, L = Ce.shape[:2]
    m = torch.arange(Q + 1)
    Ch = torch.zeros(B, L, Nh + 1, dtype=dtype)
    Sh = torch.zeros(B, L, Nh + 1, dtype=dtype)
    Mh = torch.zeros(B, L, Nh + 1, dtype=dtype)
    Ch[..., Nh - m] = Ce - Co
    Sh[..., Nh - m] = So - Se
    Ch[..., m] = Ce + Co                   # m = N/4 is written twice; the kernel takes the m <= N/4 form
    Sh[..., m] = Se + So
    mag = Ce.abs() + Co.abs() + Se.abs() + So.abs()
    Mh[..., Nh - m] = mag
    Mh[..., m] = mag
    n = torch.arange(N)
    fold = torch.where(n <= Nh, n, N - n)
    sign = torch.where(n <= Nh, -1.0, 1.0).to(dtype)
    xt = Ch[..., fold] + sign * Sh[..., fold]                      # [B][L][N]
    xm = Mh[..., fold]
    R = N // hop
    total = (L - 1) * hop + N
    acc = torch.zeros(B, total, dtype=dtype)
    amag = torch.zeros(B, total, dtype=dtype)
    emag = torch.zeros(B, total, dtype=dtype)
    env = torch.zeros(total, dtype=dtype)
    for t in (range(L - 1, -1, -1) if reverse else range(L)):
        acc[:, t * hop:t * hop + N] += xt[:, t] * win
        amag[:, t * hop:t * hop + N] += (xt[:, t] * win).abs()
        emag[:, t * hop:t * hop + N] += xm[:, t] * win.abs()
        env[t * hop:t * hop + N] += win ** 2
    pad = N // 2 if center else (N - hop) // 2
    T = hop * (L - 1) if center else hop * L
    acc, amag, emag, env = acc[:, pad:pad + T], amag[:, pad:pad + T], emag[:, pad:pad + T], env[pad:pad + T]
    y = acc / env
    # two butterfly levels on the four parts (2 ULP of their magnitudes), the window product and R accumulations; the
    # envelope is a sum of R positive terms; one division
    e = (2 * ULP * emag + (1 + dot_k(R)) * ULP * amag) / env + y.abs() * (dot_k(R) + 1) * ULP + TINY
    return y, e


# ---------------------------------------------------------------------------------------------------- small convs
def _reflect_pad_time(x, pl, pr):
    """x [B][C][T] through the reference's reflect padding (zero extension for T <= pad), by index arithmetic."""
    T = x.shape[-1]
    Tp = T if T > max(pl, pr) else max(pl, pr) + 1
    pos = torch.arange(-pl, T + pr)
    pos = torch.where(pos < 0, -pos, pos)
    pos = torch.where(pos >= Tp, 2 * (Tp - 1) - pos, pos)
    ok = pos < T
    return x[..., pos.clamp(max=T - 1)] * ok


def conv_first(wav, w, bias):
    """SConv1d(1, Cout, k) with reflect padding: wav [B][T], w [k][Cout] -> [B][T][Cout]; a chain of k multiply-adds on
    the bias."""
    k, Cout = w.shape
    pl, pr = (k - 1) - (k - 1) // 2, (k - 1) // 2
    xp = _reflect_pad_time(wav[:, None, :], pl, pr)
    wt = w.t()[:, None, :]                                                 # [Cout][1][k]
    y = F.conv1d(xp, wt, bias).transpose(1, 2)
    mag = F.conv1d(xp.abs(), wt.abs(), bias.abs()).transpose(1, 2)
    return y, dot_k(k + 1) * ULP * mag


def conv_last(x, w, bias, elu_in):
    """SConv1d(Cin, 1, k) with reflect padding and ELU on its input: x [B][T][Cin], w [k][Cin], bias [1] -> [B][T].
    Chain: a 4-element group (3), the groups of a tap row or the taps of a lane (<= 8 + 7), shuffle levels (<= 6), bias."""
    k, Cin = w.shape
    pl, pr = (k - 1) - (k - 1) // 2, (k - 1) // 2
    a = elu(x) if elu_in else x
    xp = _reflect_pad_time(a.transpose(1, 2), pl, pr)
    wt = w.t()[None]                                                       # [1][Cin][k]
    y = F.conv1d(xp, wt, bias)[:, 0]
    mag = F.conv1d(xp.abs(), wt.abs(), bias.abs())[:, 0]
    e = dot_k(26) * ULP * mag
    if elu_in:
        e = e + G.FN_ABS * w.abs().sum()
    return y, e


def convtr(x, w, bias, stride, elu_in):
    """SConvTranspose1d: x [B][T][Cin], w [k][Cin][Cout] -> [B][T stride][Cout], trimmed by k - stride (the larger half on
    the left).  Chain: every (tap, input channel) in series on the bias."""
    k, Cin, Cout = w.shape
    a = elu(x) if elu_in else x
    wt = w.permute(1, 2, 0)                                                # [Cin][Cout][k]
    full = F.conv_transpose1d(a.transpose(1, 2), wt, bias, stride=stride)
    mag = F.conv_transpose1d(a.abs().transpose(1, 2), wt.abs(), bias.abs(), stride=stride)
    tot = k - stride
    pr = tot // 2
    pl = tot - pr
    end = full.shape[-1] - pr
    y, mag = full[..., pl:end].transpose(1, 2), mag[..., pl:end].transpose(1, 2)
    taps = -(-k // stride)
    e = dot_k(taps * Cin + 1) * ULP * mag
    if elu_in:
        e = e + G.FN_ABS * taps * w.abs().sum(1).max(0).values       # <= `taps` taps of |w| summed over Cin, per output channel
    return y, e


def row_sumsq(x):
    """sum_c x^2 per row of x [rows][D]: positive terms, per-lane chains of ceil(D / 256) 4-element steps, 6 levels."""
    D = x.shape[-1]
    y = (x ** 2).sum(-1)
    return y, dot_k(4 * math.ceil(D / 256) + 8) * ULP * y + TINY
