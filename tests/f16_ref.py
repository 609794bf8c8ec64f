"""The one-product GEMM mode (WT_PLAN_FLAG_F16_GEMM, set_gemm_precision("f16")) restated from the definitions, on the CPU:
what the hi half of a split-f16 operand is, and the decoder in float64 with the operands of every contraction the decode plans
run on gemm16s rounded to those hi halves.  Nothing here comes from a kernel output."""
import math

import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ operands
def act_hi(x):
    """Hi half of an activation (split2_f16, common.h): f16(v), round to nearest even.  Any float tensor -> float64."""
    return x.to(torch.float32).to(torch.float16).to(torch.float64)


def s32_weight_scale(amax):
    """weights.cpp s32_weight_scale: 1 for a maximum inside [2^-6, 2^12) (or zero); a maximum below the window is brought into
    [1, 2), one above it into the window's top binade [2^11, 2^12); 0 where that power or its reciprocal is no normal fp32 (a
    maximum below 2^-126) or the maximum is not finite: the tensor is not split."""
    amax = float(np.float32(amax))
    if not amax > 0.0 or 2.0 ** -6 <= amax < 2.0 ** 12:
        return 1.0
    if not amax >= 2.0 ** -126 or not math.isfinite(amax):
        return 0.0
    _m, e = math.frexp(amax)
    return math.ldexp(1.0, (1 if amax < 1.0 else 12) - e)


def weight_hi(w):
    """Hi half of a weight tensor as the library stores it: f16(w s) / s with the per-tensor power of two s.  -> float64"""
    w32 = w.to(torch.float32)
    s = (s32_weight_scale(float(w32.abs().max())) if w32.numel() else 1.0) or 1.0        # 0: not split, stored as it is (add_s32)
    return (w32 * s).to(torch.float16).to(torch.float64) / s


# ------------------------------------------------------------------------------------------------ decoder emulation
def _lin(x, w, b=None, q=True):
    """x [..., K] . w [N, K]^T (+ b) in float64; with q the operands are rounded to their hi halves first."""
    y = (act_hi(x) if q else x) @ (weight_hi(w) if q else w.double()).t()
    return y if b is None else y + b.double()


def _conv(x, w, b, q=True):
    """'same' zero-padded Conv1d on x [B, C, L] as the plans run it: one contraction over (tap, channel)."""
    k = w.shape[-1]
    return F.conv1d(act_hi(x) if q else x, weight_hi(w) if q else w.double(), b.double(), padding=(k - 1) // 2)


def _swish(x):
    return x * torch.sigmoid(x)


def _gn(x, w, b):
    return F.group_norm(x, 32, w.double(), b.double(), eps=1e-6)


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w.double(), b.double(), eps=1e-6)


def istft_basis(n_fft, window):
    """The inverse real DFT with the synthesis window folded in, as one matrix: frame = [re | im] @ basis, basis [2 (n_fft/2+1), n_fft]."""
    n = torch.arange(n_fft, dtype=torch.float64)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)
    ang = 2.0 * math.pi * k[:, None] * n[None, :] / n_fft
    wk = torch.full((n_fft // 2 + 1,), 2.0, dtype=torch.float64)
    wk[0] = 1.0
    wk[-1] = 1.0
    c = wk[:, None] * torch.cos(ang) / n_fft
    s = -wk[:, None] * torch.sin(ang) / n_fft
    s[0] = 0.0
    s[-1] = 0.0
    return torch.cat([c, s], 0) * window.double()[None, :]


def decode_f64(arch, sd, features, bw, q):
    """The decoder (backbone + ISTFT head) in float64 on features [B, C, L].  q = False: the plain float64 run.  q = True: the
    operands of every contraction that build_decode + plan_head run on gemm16s are rounded to their hi halves (activations
    f16(v), weights f16(w s) / s): embed, the eight k3 convs, q|k, V^T, scores, P.V, proj, the 24 ConvNeXt linears, the head
    linear and the inverse DFT (an explicit product with the window . cos/sin / n basis, rounded like a weight).  The depthwise
    conv, the norms, softmax and the element-wise maths are not touched."""
    g = lambda k: torch.as_tensor(sd[k])
    x = _conv(features.double(), g("backbone.embed.weight"), g("backbone.embed.bias"), q)

    def resnet(x, p):
        h = _swish(_gn(x, g(p + "norm1.weight"), g(p + "norm1.bias")))
        h = _conv(h, g(p + "conv1.weight"), g(p + "conv1.bias"), q)
        h = _swish(_gn(h, g(p + "norm2.weight"), g(p + "norm2.bias")))
        h = _conv(h, g(p + "conv2.weight"), g(p + "conv2.bias"), q)
        return x + h

    x = resnet(x, "backbone.pos_net.0.")
    x = resnet(x, "backbone.pos_net.1.")
    p = "backbone.pos_net.2."
    h = _gn(x, g(p + "norm.weight"), g(p + "norm.bias")).transpose(1, 2)            # [B, L, D]
    D = h.shape[-1]
    qq = _lin(h, g(p + "q.weight")[:, :, 0], g(p + "q.bias"), q)
    kk = _lin(h, g(p + "k.weight")[:, :, 0], g(p + "k.bias"), q)
    vv = _lin(h, g(p + "v.weight")[:, :, 0], g(p + "v.bias"), q)
    if q:       # q | k, V^T and the probabilities are written split by their producers: the next product reads their hi halves
        qq, kk, vv = act_hi(qq), act_hi(kk), act_hi(vv)
    sc = torch.matmul(qq, kk.transpose(1, 2)) * float(D) ** -0.5
    pr = torch.softmax(sc, dim=-1)
    o = torch.matmul(act_hi(pr) if q else pr, vv)
    x = x + _lin(o, g(p + "proj_out.weight")[:, :, 0], g(p + "proj_out.bias"), q).transpose(1, 2)
    x = resnet(x, "backbone.pos_net.3.")
    x = resnet(x, "backbone.pos_net.4.")
    x = _gn(x, g("backbone.pos_net.5.weight"), g("backbone.pos_net.5.bias"))
    x = x.transpose(1, 2)                                                         # [B, L, D]

    def adanorm(x, p):
        y = F.layer_norm(x, (x.shape[-1],), eps=1e-6)
        return y * g(p + "scale.weight")[bw].double() + g(p + "shift.weight")[bw].double()

    x = adanorm(x, "backbone.norm.")
    i = 0
    while f"backbone.convnext.{i}.dwconv.weight" in sd:
        p = f"backbone.convnext.{i}."
        r = x
        h = F.conv1d(x.transpose(1, 2), g(p + "dwconv.weight").double(), g(p + "dwconv.bias").double(), padding=3, groups=x.shape[-1])
        h = adanorm(h.transpose(1, 2), p + "norm.")
        h = _lin(h, g(p + "pwconv1.weight"), g(p + "pwconv1.bias"), q)
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        h = _lin(h, g(p + "pwconv2.weight"), g(p + "pwconv2.bias"), q)
        x = r + g(p + "gamma").double() * h
        i += 1
    x = _ln(x, g("backbone.final_layer_norm.weight"), g("backbone.final_layer_norm.bias"))
    # ISTFTHead (heads.py:53-66) and ISTFT (spectral_ops.py:56-73)
    y = _lin(x, g("head.out.weight"), g("head.out.bias"), q)
    n_fft, hop = arch.n_fft, arch.hop_length
    nb = n_fft // 2 + 1
    mag = torch.clamp(torch.exp(y[..., :nb]), max=100.0)
    ph = y[..., nb:]
    spec = torch.cat([mag * torch.cos(ph), mag * torch.sin(ph)], -1)              # [B, L, 2 nb]
    window = g("head.istft.window")
    basis = istft_basis(n_fft, window)
    frames = (act_hi(spec) if q else spec) @ (weight_hi(basis) if q else basis)     # [B, L, n_fft], windowed
    B, L, _ = frames.shape
    out_len = (L - 1) * hop + n_fft
    fold = lambda t: F.fold(t.transpose(1, 2), output_size=(1, out_len), kernel_size=(1, n_fft), stride=(1, hop))[:, 0, 0, :]
    yw = fold(frames)
    env = fold((window.double() ** 2).expand(1, L, -1))
    if arch.padding == "same":
        pad = (n_fft - hop) // 2
        return yw[:, pad:out_len - pad] / env[:, pad:out_len - pad]
    pad = n_fft // 2
    return yw[:, pad:out_len - pad] / env[:, pad:out_len - pad]


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b) ** 2).sum().sqrt() / (b ** 2).sum().sqrt())
