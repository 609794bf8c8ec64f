"""Float64 references and per-element error bounds for the fused encoder kernels of csrc/resblock16.hip and csrc/resblock.hip
(tests/test_encoder_ops.py and tests/test_encoder_ops_mixed.py on the GPU, tests/test_enc_checks.py on the CPU).  Everything
is written from the definitions the kernel comments cite, never from a kernel output: SEANetResnetBlock (seanet.py:21-63:
y = shortcut(x) + conv1(elu(conv3(elu(x))))), the encoder's first conv and a stage's ELU + strided conv (seanet.py:107-127),
SConv1d's reflect padding with the extra right padding that completes the last window and the zero extension of inputs shorter
than the pad (conv.py:54-61, 79-96, 195-211; oracle.cpu_ref restates the two helpers).  Weight norm is folded in float64.  CPU only.

Every reference returns (ref, bound), time-major [clip][frame][channel].  The bound is propagated through the fused chain, not
set per tensor.  On the split-f16 chain of resblock16.hip (TOL = tol16(K) per contraction relative to sum |a w|: gemm_ref.TOL's
derivation at the contraction's own K; gemm_ref's S32_ENC for a value re-encoded as hi + lo 2^-11, ABS_FLOOR for the f16
subnormal floor of lo, ULP for an fp32 rounding):

  first conv    K = 8: seven taps and the bias as the eighth K slot against a constant 1:  e_x = TOL (sum |w wav| + |b0|)
  ELU           e_a = e_x max|elu'| + elu_err + the re-encoding of elu(x): the slope is e^min(0, x + e_x) <= 1, the function's
                own error at most 2 ULP (elu_err; gemm_ref.FN_ABS = 1e-6 is that figure with a margin of 4)
  k3 conv       the incoming error goes through |W3| with the conv's own padding; TOL sum |a w| for the contraction
  ELU           again, on the hidden activation
  output        shortcut and conv1 in ONE accumulation (K = C/2 + C) with b1 + bs: |W1| e_g + TOL (sum |W1 g| + sum |Ws x| +
                |b1 + bs|).  With the first conv folded in, the shortcut is the 8-slot product (Ws E0 | Ws b0 + b1 + bs) .
                (wav, 1): its magnitude is that of this form, the reference value is the definition's
  elu_out, S32  optional ELU and encoding of the stored value
  DOWN          ELU (re-encoded), then the strided reflect conv: the error goes through |Wd| with that conv's padding

F32 is the same propagation for the fp32 chain of resblock.hip: products are exact, a contraction of K terms accumulated in
series is within (K + 2) 2^-24 of sum |a w|, nothing is re-encoded, and the shortcut reads the first conv's fp32 output."""
import torch
import torch.nn.functional as F

from oracle.cpu_ref import get_extra_padding_for_conv1d, pad1d_reflect
from tests import gemm_ref as G

ULP = G.ULP
U = 2.0 ** -24                   # fp32 unit roundoff


class Chain:
    """Arithmetic of a kernel family: tol(K) per contraction, enc / floor of a re-encoded intermediate, and whether the folded
    first conv carries the shortcut (resblock16.hip) or the shortcut reads the first conv's output (resblock.hip)."""

    def __init__(self, name, tol, enc, floor, fold_shortcut):
        self.name, self.tol, self.enc, self.floor, self.fold_shortcut = name, tol, enc, floor, fold_shortcut


def tol16(K, encoded=False):
    """gemm_ref.TOL is sized for K <= 2304 with a margin of 3; the fused chain stacks four contractions of K <= 256, and a bound
    that wide lets a dropped lo half through (tests/test_enc_checks.py).  The same derivation at the K of each contraction,
    without the margin: 2^-22 for each operand's split and for the dropped lo.lo product, and one fp32 rounding per 16-deep
    MFMA step of the accumulation plus five for joining the main and the correction accumulator, the 2^-11 scale and the bias.
    encoded: the activation operand is an intermediate whose split act() has charged already."""
    return min(G.TOL, ((2 if encoded else 3) + (K / 16 + 5) / 4) * 2.0 ** -22)


S16 = Chain("split-f16", tol16, G.S32_ENC, G.ABS_FLOOR, True)
F32 = Chain("fp32", lambda K, encoded=False: (K + 2) * U, 0.0, 0.0, False)


def fold_weight_norm(g, v):
    """weight_norm (conv.py:25-34) in float64: w = g v / ||v|| per output channel; returns the fp32 values the kernels get, as
    float64 [Cout][Cin][k]."""
    g, v = torch.as_tensor(g).double(), torch.as_tensor(v).double()
    w = g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
    return w.float().double()


ENC = "feature_extractor.encodec.encoder.model."


def stage_weights(sd, stage, down=None):
    """The folded weights of encoder resblock `stage` (1, 4, ...) of a state dict, with the first conv and, for down = the index
    of the stage's strided conv, that conv: float64 copies of the fp32 values, conv layout [Cout][Cin][k]."""
    def conv(prefix):
        return (fold_weight_norm(sd[prefix + ".weight_g"], sd[prefix + ".weight_v"]), torch.as_tensor(sd[prefix + ".bias"]).double())
    W = {}
    W["e0w"], W["e0b"] = conv(ENC + "0.conv.conv")
    W["w3"], W["b3"] = conv(ENC + f"{stage}.block.1.conv.conv")
    W["w1"], W["b1"] = conv(ENC + f"{stage}.block.3.conv.conv")
    W["ws"], W["bs"] = conv(ENC + f"{stage}.shortcut.conv.conv")
    if down is not None:
        W["wd"], W["bd"] = conv(ENC + f"{down}.conv.conv")
    return W


def sconv_pad(x, k, stride):
    """SConv1d's padding of x [..][T], non-causal (conv.py:195-211): reflect by (k - stride) split with the larger half on the
    left, plus the extra right padding that completes the last window (conv.py:54-61)."""
    pt = k - stride
    extra = get_extra_padding_for_conv1d(x.shape[-1], k, stride, pt)
    pr = pt // 2
    return pad1d_reflect(x, (pt - pr, pr + extra))


def sconv(x, e_x, w, b, stride, tol, floor):
    """SConv1d on x [B][Cin][T] known to e_x (None: exact): (y, e_y, mag) with mag = sum |w x| + |b|."""
    k = w.shape[-1]
    xp = sconv_pad(x, k, stride)
    y = F.conv1d(xp, w, b, stride=stride)
    mag = F.conv1d(xp.abs(), w.abs(), b.abs(), stride=stride)
    e = tol * mag + floor + ULP * y.abs()
    if e_x is not None:
        e = e + F.conv1d(sconv_pad(e_x, k, stride), w.abs(), None, stride=stride)
    return y, e, mag


def elu_err(v, e_v):
    """Absolute error of the kernels' ELU, x > 0 ? x : exp2(x log2 e) - 1 (common.h elu_med3; resblock.hip: __expf), at an
    argument known to e_v.  The median form returns x once the computed e^x - 1 is above x for certain (x^2 / 2 beyond two
    roundings of a number near 1: x > 1e-3 is far enough), with no error.  Below that v_exp_f32 is within 1 ulp of a result
    e^x <= 1 and the rounded product x log2 e moves the exponent by at most |x| 2^-24 (tests/op_ref.py exp_rel: (2 + |x|) ULP
    relative to e^x <= 1.001); the rounding of the subtraction is relative to the result and is added by the caller.  Never above
    2 ULP = 2.4e-7, the figure gemm_ref.FN_ABS = 1e-6 covers with a margin that three stacked ELUs cannot afford."""
    e = 0.0 if e_v is None else e_v
    return torch.where(v - e > 1e-3, torch.zeros_like(v), (2 + v.abs()) * torch.exp(v.clamp(max=1e-3)) * ULP)


def act(v, e_v, ch):
    """ELU of a value known to e_v, stored as an operand of the next contraction (re-encoded on the split-f16 chain).  The
    incoming error passes through the largest slope ELU has between v and v +- e_v: e^min(0, v + e_v) <= 1."""
    a = G.elu(v)
    e = elu_err(v, e_v) + ULP * a.abs() + ch.enc * a.abs() + ch.floor
    return a, (e if e_v is None else e + e_v * torch.exp((v + e_v).clamp(max=0.0)))


def resblock(W, x=None, wav=None, elu_out=0, out_s32=0, down=0, chain=S16):
    """The fused block on x [B][C][T] (float64 copies of fp32 values) or, with wav [B][T], on the first conv of the waveform;
    down = r: followed by ELU and the stage's strided conv, whose output [B][ceil(T / r)][64] is then the result.
    (ref, bound), time-major."""
    ch = chain
    e_x = None
    if wav is not None:
        x, e_x, _ = sconv(wav[:, None, :], None, W["e0w"], W["e0b"], 1, ch.tol(8), ch.floor)
    C = x.shape[1]
    H = C // 2
    a, e_a = act(x, e_x, ch)
    h, e_h, _ = sconv(a, e_a, W["w3"], W["b3"], 1, ch.tol(3 * C, True), ch.floor)
    g, e_g = act(h, e_h, ch)
    b12 = W["b1"] + W["bs"]
    y = F.conv1d(g, W["w1"]) + F.conv1d(x, W["ws"]) + b12[:, None]
    e_y = F.conv1d(e_g, W["w1"].abs())
    mag = F.conv1d(g.abs(), W["w1"].abs())
    if wav is not None and ch.fold_shortcut:
        # the shortcut as the kernel forms it: (Ws E0)[n][j] and Ws b0 + b1 + bs in double, rounded to fp32, one 8-slot product
        v = torch.einsum("nc,cj->nj", W["ws"][:, :, 0], W["e0w"][:, 0, :]).float().double()
        v7 = (W["ws"][:, :, 0] @ W["e0b"] + b12).float().double()
        mag = mag + F.conv1d(sconv_pad(wav[:, None, :], 7, 1).abs(), v.abs()[:, None, :]) + v7.abs()[:, None]
        K = 8 + H
    else:
        mag = mag + F.conv1d(x.abs(), W["ws"].abs()) + b12.abs()[:, None]
        if e_x is not None:
            e_y = e_y + F.conv1d(e_x, W["ws"].abs())
        K = H + C
    e_y = e_y + ch.tol(K) * mag + ch.floor + ULP * (y.abs() + b12.abs()[:, None])
    if down:
        z, e_z = act(y, e_y, ch)
        d, e_d, _ = sconv(z, e_z, W["wd"], W["bd"], down, ch.tol(2 * down * C, True), ch.floor)
        return d.transpose(1, 2), e_d.transpose(1, 2)
    if elu_out:
        e_y = e_y * torch.exp((y + e_y).clamp(max=0.0)) + elu_err(y, e_y)
        y = G.elu(y)
        e_y = e_y + ULP * y.abs()
    if out_s32:
        e_y = e_y + G.S32_ENC * y.abs() + G.ABS_FLOOR
    return y.transpose(1, 2), e_y.transpose(1, 2)
