"""The weights as wt_model_create leaves them in HBM, restated from the raw state dict in float64 / long double numpy, and the
checker that compares a set of loaded arrays (tests/test_model_weights.py reads them from the device through
wt_model_weight_info; tests/test_weight_checks.py makes them on the CPU, honestly and with deliberate slips) with it.
Nothing here comes from a kernel output.

Bounds (derived, not tuned):
  split       |v - (hi + lo 2^-11)| <= max(2^-22 |v|, 2^-36) for finite |v| < 65504: hi = f16(v) leaves a remainder of at most
              half an f16 ulp of v, 2^-11 |v| (2^-25 below the f16 normal range); lo = f16(remainder 2^11) rounds that to 11
              bits, 2^-11 of it, and has the f16 subnormal spacing 2^-24 as its absolute floor: 2^-25 2^-11 = 2^-36.
  fold        the library forms g / sqrt(sum v^2) and the product in double, then casts once: one fp32 rounding (2^-24) and
              inner + 8 double roundings (the running sum's inner, and sqrt, divide, multiply, conversions).
  ee          fp32 running sum of 512 non-negative squares: 512 roundings, each at most 2^-24 of the final sum.
  basis       c cos(theta) in double with theta = 2 pi (f n mod N) / N: the angle carries a few double roundings (< 2 pi 2^-52
              absolute, which is what the cosine can move by: c 2^-50 with margin), the product two more (2^-50 |ref| with margin),
              then one cast (2^-24 |ref|).
  everything else is a permutation, a concatenation or one fp32 addition of raw tensors: bit-exact."""
import numpy as np
import torch

from tests import f16_ref, gemm_ref, lstm_ref

F32, S32, LSTM_F16, LSTM_PERSIST = 0, 1, 2, 3          # wt_weight_info.format
ENC = "feature_extractor.encodec.encoder.model."
DEC = "feature_extractor.encodec.decoder.model."
VQ = "feature_extractor.encodec.quantizer.vq.layers.%d._codebook."
U24, U53 = 2.0 ** -24, 2.0 ** -53
H = 512
NF = 32


# ------------------------------------------------------------------------------------------------ the split form
def split_emulate(v):
    """fp32 [n] (n % 32 == 0) -> uint16 [2 n]: the S32 encoding of v.  hi = float16(v), lo = float16((v - float32(hi)) * 2048),
    both round to nearest even; hi of element i at g = (i >> 5) * 64 + (i & 31), lo at g + 32."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    assert v.size % 32 == 0
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return np.stack([hi.reshape(-1, 32), lo.reshape(-1, 32)], 1).reshape(-1).view(np.uint16)


def split_halves(words):
    """uint16 [2 n] in the S32 layout -> (hi, lo) float16 [n] each."""
    h = np.ascontiguousarray(words).view(np.float16).reshape(-1, 2, 32)
    return h[:, 0, :].reshape(-1), h[:, 1, :].reshape(-1)


def split_value(words):
    """uint16 [2 n] -> float64 [n]: hi + lo 2^-11."""
    hi, lo = split_halves(words)
    with np.errstate(invalid="ignore"):                   # (inf - inf of an over-range value)
        return hi.astype(np.float64) + lo.astype(np.float64) / 2048.0


def split_value_f32(words, inv_scale=1.0):
    """unsplit_s32_kernel: (float32(hi) + float32(lo) * (1 / 2048)) * inv_scale in fp32."""
    hi, lo = split_halves(words)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (hi.astype(np.float32) + lo.astype(np.float32) * np.float32(1.0 / 2048.0)) * np.float32(inv_scale)


def split_bound(v):
    """The float64 bound on |v - (hi + lo 2^-11)|, for finite |v| < 65504."""
    return np.maximum(2.0 ** -22 * np.abs(np.asarray(v, np.float64)), 2.0 ** -36)


def words_match(got, want, hi=None):
    """bool per f16 half (uint16 views): equal bit for bit, a NaN half matching any NaN half.  hi: bool per half, True where it
    is a hi half; there, and only there, an expected -0 may come back as +0: for hi = (_Float16)(x * sc) the compiler selects one
    v_fma_mixlo_f16 with a +0 addend (product and conversion in one rounding), and (-0) sc + (+0) is +0."""
    got, want = np.asarray(got).view(np.uint16), np.asarray(want).view(np.uint16)
    nan = lambda a: (a & 0x7fff) > 0x7c00
    ok = (got == want) | (nan(got) & nan(want))
    if hi is not None:
        ok = ok | (hi & (want == 0x8000) & (got == 0x0000))
    return ok


def same_words(got, want, s32=False):
    """Both flat uint16 arrays: every half matches (words_match); s32: they are in the S32 layout, whose hi halves are the
    first 32 of every 64."""
    got, want = np.asarray(got).view(np.uint16).reshape(-1), np.asarray(want).view(np.uint16).reshape(-1)
    if got.shape != want.shape:
        return False
    hi = (np.arange(got.size) & 32) == 0 if s32 else None
    return bool(np.all(words_match(got, want, hi)))


def tap_pair_order(k, r):
    return gemm_ref.tap_order(k, r, True)


# ------------------------------------------------------------------------------------------------ references
class Ref:
    """One loaded array.  kind "exact": `ref` (fp32 or uint16) bit for bit; "bound": float64 `ref` within `bound`;
    "derived": fn(get) -> the fp32 array bit for bit, with get(name) = a loaded array (a rearrangement of loaded arrays)."""
    def __init__(self, kind, ref=None, bound=None, cls="perm", fn=None, fmt=F32):
        self.kind, self.ref, self.bound, self.cls, self.fn, self.fmt = kind, ref, bound, cls, fn, fmt


def _exact(a, cls="perm", fmt=F32):
    return Ref("exact", np.ascontiguousarray(a), cls=cls, fmt=fmt)


def fold_ref(g, v):
    """weight_norm over dim 0 of v (every other axis is summed), norm summed in long double: (float64 ref, bound) in v's shape."""
    v = np.asarray(v, np.float32)
    g = np.asarray(g, np.float32).reshape(-1)
    flat = v.reshape(v.shape[0], -1).astype(np.longdouble)
    norm = np.sqrt((flat * flat).sum(1))
    ref = ((g.astype(np.longdouble) / norm)[:, None] * flat).astype(np.float64).reshape(v.shape)
    inner = flat.shape[1]
    return ref, (U24 + (inner + 8) * U53) * np.abs(ref)


def _conv_wn(sd, prefix, out, name):
    ref, bound = fold_ref(sd[prefix + ".weight_g"], sd[prefix + ".weight_v"])
    out[name + ".w"] = Ref("bound", ref.transpose(0, 2, 1), bound.transpose(0, 2, 1), cls="fold")       # [cout][k][cin]
    out[name + ".b"] = _exact(sd[prefix + ".bias"])


def _conv_plain(sd, prefix, out, name):
    w = np.asarray(sd[prefix + ".weight"], np.float32)
    out[name + ".w"] = _exact(w.transpose(0, 2, 1))
    out[name + ".b"] = _exact(sd[prefix + ".bias"])


def lstm_packings(wih0, whh0, wih1, whh1, bih0, bhh0, bih1, bhh1):
    """weights.cpp load_lstm in numpy: {suffix: array}.  Rows go to the packed gate order (lstm_ref.pack_gates); the recurrent
    weights to the three lane packings, the f16 ones as hi = f16(w), lo = f16((w - hi) 2048), unscaled."""
    def rows(w):                                     # [4 H][K] -> packed rows
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(w, np.float32).reshape(4, H, -1).transpose(2, 0, 1)))     # [K][4][H]
        return lstm_ref.pack_gates(t).numpy().T.copy()

    def vec(b):
        return lstm_ref.pack_gates(torch.from_numpy(np.asarray(b, np.float32).reshape(4, H).copy())).numpy()

    def halves(x):
        with np.errstate(over="ignore", invalid="ignore"):
            hi = x.astype(np.float16)
            lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
        return hi, lo

    def lanes32(w):                                  # element e of group S, lane (lk, li): W[16 blk + li][16 S + 4 e + lk]
        K = w.shape[1]
        return w.reshape(-1, 16, K // 16, 4, 4).transpose(0, 2, 4, 1, 3).copy()

    def lanes16(w):                                  # half p = 4 a + b of lane (lk, li) in block P: W[16 blk + li][32 P + 16 a + 4 b + lk]
        K = w.shape[1]
        hi, lo = (t.reshape(-1, 16, K // 32, 2, 4, 4).transpose(0, 2, 5, 1, 3, 4) for t in halves(w))
        return np.stack([hi, lo], 2).copy().view(np.uint16)

    def lanes_persist(ws):                           # [role][wg][tile][blk][hi, lo][lk][li][p]: W[64 wg + 16 tile + li][32 blk + 8 lk + p]
        out = []
        for w in ws:
            hi, lo = (t.reshape(32, 4, 16, 16, 4, 8).transpose(0, 1, 3, 4, 2, 5) for t in halves(w))
            out.append(np.stack([hi, lo], 3))
        return np.stack(out, 0).copy().view(np.uint16)

    W0 = rows(whh0)
    W1 = np.concatenate([rows(wih1), rows(whh1)], 1)
    return {"Wih0": rows(wih0), "b0": vec(np.asarray(bih0, np.float32) + np.asarray(bhh0, np.float32)),
            "W0": lanes32(W0), "W1": lanes32(W1), "b1": vec(np.asarray(bih1, np.float32) + np.asarray(bhh1, np.float32)),
            "W0h": lanes16(W0), "W1h": lanes16(W1), "Wp": lanes_persist([W0, rows(wih1), rows(whh1)])}


def _lstm(sd, prefix, out, name):
    k = lambda s: sd[prefix + ".lstm." + s]
    p = lstm_packings(k("weight_ih_l0"), k("weight_hh_l0"), k("weight_ih_l1"), k("weight_hh_l1"),
                      k("bias_ih_l0"), k("bias_hh_l0"), k("bias_ih_l1"), k("bias_hh_l1"))
    for s, a in p.items():
        fmt = {"W0h": LSTM_F16, "W1h": LSTM_F16, "Wp": LSTM_PERSIST}.get(s, F32)
        out[name + "." + s] = _exact(a, fmt=fmt)


def head_slots(n_fft):
    """(Kq, Kb, bin of spectrum slot s or -1): even bins 2 s for s < Kq, odd bins 2 (s - Kq) + 1 behind them, padded to 32."""
    Q = n_fft // 4
    Kq = (Q + 1 + 31) // 32 * 32
    bins = []
    for s in range(2 * Kq):
        f = 2 * s if s < Kq else 2 * (s - Kq) + 1
        bins.append(f if f <= n_fft // 2 and (s < Kq or s - Kq < Q) else -1)
    return Kq, 2 * Kq, bins


def head_rows(w, b, n_fft):
    """head.out weight [n_fft + 2][D] and bias -> the packed [2 Kb][D] rows and [2 Kb] bias (gemm_ref.pack_head_rows; pad rows 0)."""
    Kq, Kb, bins = head_slots(n_fft)
    nb = n_fft // 2 + 1
    w = np.asarray(w, np.float32).reshape(n_fft + 2, -1)
    b = np.asarray(b, np.float32)
    lm = np.zeros((Kb, w.shape[1] + 1), np.float32)
    ph = np.zeros_like(lm)
    for s, f in enumerate(bins):
        if f >= 0:
            lm[s, :-1], lm[s, -1] = w[f], b[f]
            ph[s, :-1], ph[s, -1] = w[nb + f], b[nb + f]
    packed = gemm_ref.pack_head_rows(torch.from_numpy(lm), torch.from_numpy(ph)).numpy()
    return packed[:, :-1].copy(), packed[:, -1].copy()


def dft_basis(n_fft):
    """The four quarter bases [4][Kq][Kq] (Re even, Re odd, Im even, Im odd bins; row n, column g) in long double, and the bound."""
    N, Q = n_fft, n_fft // 4
    Kq = head_slots(n_fft)[0]
    ld = np.longdouble
    two_pi = 2 * np.arctan2(ld(0), ld(-1))
    n = np.arange(Q + 1)[:, None]
    g = np.arange(Q + 1)[None, :]
    ref = np.zeros((4, Kq, Kq), np.float64)
    c = np.zeros((4, Kq, Kq), np.float64)
    fe, fo = 2 * g, 2 * g + 1
    edge = (fe == 0) | (fe == N // 2)
    ce = np.where(edge, 1.0, 2.0) / N
    co = 2.0 / N
    the = two_pi * ((fe * n) % N).astype(ld) / ld(N)
    tho = two_pi * ((fo * n) % N).astype(ld) / ld(N)
    ref[0, :Q + 1, :Q + 1] = (ce * np.cos(the)).astype(np.float64)
    ref[2, :Q + 1, :Q + 1] = np.where(edge, 0.0, (ce * np.sin(the)).astype(np.float64))
    ref[1, :Q + 1, :Q] = (co * np.cos(tho)).astype(np.float64)[:, :Q]
    ref[3, :Q + 1, :Q] = (co * np.sin(tho)).astype(np.float64)[:, :Q]
    c[0, :Q + 1, :Q + 1] = c[2, :Q + 1, :Q + 1] = np.broadcast_to(ce, (Q + 1, Q + 1))
    c[2, :Q + 1, :Q + 1][np.broadcast_to(edge, (Q + 1, Q + 1))] = 0.0          # Im of DC and Nyquist: exactly 0
    c[1, :Q + 1, :Q] = c[3, :Q + 1, :Q] = co
    return ref, (U24 + 2.0 ** -50) * np.abs(ref) + c * 2.0 ** -50              # outside the computed block: ref = bound = 0


def fusable(C):
    return C in (32, 64)


def expected(arch, sd):
    """{name: Ref} of every fp32 array and LSTM packing a model of `arch` loaded from `sd` holds (the S32 copies follow from the
    loaded fp32 arrays: expected_copies)."""
    out = {}
    D, A, N = arch.dim, arch.adanorm_num_embeddings, arch.n_fft
    ref, bound = fold_ref(sd[ENC + "0.conv.conv.weight_g"], sd[ENC + "0.conv.conv.weight_v"])      # [32][1][7]
    out["enc.e0.w"] = Ref("bound", ref[:, 0, :].T, bound[:, 0, :].T, cls="fold")
    out["enc.e0.b"] = _exact(sd[ENC + "0.conv.conv.bias"])
    idx, C = 1, NF
    for i, r in enumerate(arch.enc_ratios):
        p, s = ENC + str(idx), "enc.stage%d" % (i + 1)
        _conv_wn(sd, p + ".block.1.conv.conv", out, s + ".c3")
        _conv_wn(sd, p + ".block.3.conv.conv", out, s + ".c1")
        _conv_wn(sd, p + ".shortcut.conv.conv", out, s + ".sc")
        _conv_wn(sd, ENC + "%d.conv.conv" % (idx + 2), out, s + ".down")
        if 2 * r <= 32:
            out[s + ".down.wpair"] = Ref("derived", fn=lambda get, s=s, r=r: get(s + ".down.w")[:, tap_pair_order(2 * r, r), :])
        if not fusable(C):
            _cat(sd, p, out, s)
        idx, C = idx + 3, 2 * C
    _lstm(sd, ENC + str(idx), out, "enc.lstm")
    _conv_wn(sd, ENC + "%d.conv.conv" % (idx + 2), out, "enc.final")
    books = [np.asarray(sd[(VQ % q) + "embed"], np.float32) for q in range(arch.num_quantizers)]
    out["vq.embed"] = _exact(np.stack(books, 0))
    ee = (books[0].astype(np.float64) ** 2).sum(1)
    out["vq.ee"] = Ref("bound", ee, 512 * U24 * ee, cls="ee")
    _conv_plain(sd, "backbone.embed", out, "bb.embed")
    for i, ri in enumerate((0, 1, 3, 4)):
        p, s = "backbone.pos_net.%d" % ri, "bb.res.%d" % i
        for a, b in (("n1w", "norm1.weight"), ("n1b", "norm1.bias"), ("n2w", "norm2.weight"), ("n2b", "norm2.bias")):
            out[s + "." + a] = _exact(sd[p + "." + b])
        _conv_plain(sd, p + ".conv1", out, s + ".c1")
        _conv_plain(sd, p + ".conv2", out, s + ".c2")
    p = "backbone.pos_net.2."
    flat = lambda k: np.asarray(sd[k], np.float32).reshape(D, D)
    out["bb.attn.nw"], out["bb.attn.nb"] = _exact(sd[p + "norm.weight"]), _exact(sd[p + "norm.bias"])
    out["bb.attn.Wqk"] = _exact(np.concatenate([flat(p + "q.weight"), flat(p + "k.weight")], 0))
    out["bb.attn.bqk"] = _exact(np.concatenate([sd[p + "q.bias"], sd[p + "k.bias"]]))
    out["bb.attn.Wv"], out["bb.attn.bv"] = _exact(flat(p + "v.weight")), _exact(sd[p + "v.bias"])
    out["bb.attn.Wp"], out["bb.attn.bp"] = _exact(flat(p + "proj_out.weight")), _exact(sd[p + "proj_out.bias"])
    out["bb.gn5.w"], out["bb.gn5.b"] = _exact(sd["backbone.pos_net.5.weight"]), _exact(sd["backbone.pos_net.5.bias"])
    out["bb.ada.s"], out["bb.ada.h"] = _exact(sd["backbone.norm.scale.weight"]), _exact(sd["backbone.norm.shift.weight"])
    for i in range(arch.num_layers):
        p, s = "backbone.convnext.%d." % i, "bb.cnx.%d." % i
        out[s + "dw_w"] = _exact(np.asarray(sd[p + "dwconv.weight"], np.float32).reshape(D, 7).T)
        for a, b in (("dw_b", "dwconv.bias"), ("ada_s", "norm.scale.weight"), ("ada_h", "norm.shift.weight"), ("W1", "pwconv1.weight"),
                     ("b1", "pwconv1.bias"), ("W2", "pwconv2.weight"), ("b2", "pwconv2.bias"), ("gamma", "gamma")):
            out[s + a] = _exact(sd[p + b])
    out["bb.fln.w"], out["bb.fln.b"] = _exact(sd["backbone.final_layer_norm.weight"]), _exact(sd["backbone.final_layer_norm.bias"])
    hw, hb = head_rows(sd["head.out.weight"], sd["head.out.bias"], N)
    out["head.W"], out["head.b"] = _exact(hw, cls="head"), _exact(hb, cls="head")
    bref, bbound = dft_basis(N)
    out["istft.W"] = Ref("bound", bref, bbound, cls="basis")
    win = np.asarray(sd["head.istft.window"], np.float32)
    out["istft.win"], out["istft.wsq"] = _exact(win), _exact(win * win)
    if DEC + "0.conv.conv.weight_v" in sd:
        _conv_wn(sd, DEC + "0.conv.conv", out, "sd.first")
        _lstm(sd, DEC + "1", out, "sd.lstm")
        di, cin = 2, NF << len(arch.ratios)
        for i, r in enumerate(arch.ratios):
            p, s = DEC + "%d.convtr.convtr" % (di + 1), "sd.stage%d" % (i + 1)
            ref, bound = fold_ref(sd[p + ".weight_g"], sd[p + ".weight_v"])          # [cin][cout][k], g per cin
            out[s + ".tr_w"] = Ref("bound", ref.transpose(2, 0, 1), bound.transpose(2, 0, 1), cls="fold")
            # [phase][cout][tap][cin]: tap 0 <- kernel index phase + r, tap 1 <- phase
            out[s + ".tr_wp"] = Ref("derived", fn=lambda get, s=s, r=r: np.stack([get(s + ".tr_w")[r:2 * r], get(s + ".tr_w")[:r]], 1).transpose(0, 3, 1, 2))
            out[s + ".tr_b"] = _exact(sd[p + ".bias"])
            rp, h = DEC + str(di + 2), cin // 2
            _conv_wn(sd, rp + ".block.1.conv.conv", out, s + ".c3")
            _conv_wn(sd, rp + ".block.3.conv.conv", out, s + ".c1")
            _conv_wn(sd, rp + ".shortcut.conv.conv", out, s + ".sc")
            if not fusable(h):
                _cat(sd, rp, out, s)
            di, cin = di + 3, h
        p = DEC + "%d.conv.conv" % (di + 1)
        ref, bound = fold_ref(sd[p + ".weight_g"], sd[p + ".weight_v"])              # [1][32][7]
        out["sd.last.w"] = Ref("bound", ref[0].T, bound[0].T, cls="fold")
        out["sd.last.b"] = _exact(sd[p + ".bias"])
    return out


def _cat(sd, p, out, s):
    """[Ws | W1] of the loaded 1x1 convs, and bs + b1 in fp32."""
    out[s + ".cat.w"] = Ref("derived", fn=lambda get, s=s: np.concatenate([get(s + ".sc.w")[:, 0, :], get(s + ".c1.w")[:, 0, :]], 1)[:, None, :])
    out[s + ".cat.b"] = _exact(np.asarray(sd[p + ".shortcut.conv.conv.bias"], np.float32) + np.asarray(sd[p + ".block.3.conv.conv.bias"], np.float32))


# which arrays carry an S32 copy, in which tap order, and which a packed image leaves out (weights.cpp build_splits)
def copy_rules(arch, names):
    """{fp32 name: (tap_pair stride or 0, lazy)} of the arrays that must have an S32 copy, given the set of loaded names."""
    rules = {}
    C = NF
    for i, r in enumerate(arch.enc_ratios):
        s = "enc.stage%d" % (i + 1)
        fused = fusable(C)
        rules[s + ".down.w"] = (r if 2 * r <= 32 else 0, 0)
        rules[s + ".c3.w"] = (0, 0 if fused else 1)
        if (C // 2) % 32 == 0:
            rules[s + ".c1.w"] = (0, 0 if fused else 1)
        rules[s + ".sc.w"] = (0, 0 if fused else 1)
        if not fused:
            rules[s + ".cat.w"] = (0, 1)
        C *= 2
    for n in ["enc.lstm.Wih0", "enc.final.w", "bb.embed.w", "head.W", "istft.W", "bb.attn.Wqk", "bb.attn.Wv", "bb.attn.Wp"]:
        rules[n] = (0, 1)
    rules["vq.embed"] = (0, 0)
    for i in range(4):
        rules["bb.res.%d.c1.w" % i] = rules["bb.res.%d.c2.w" % i] = (0, 1)
    for i in range(arch.num_layers):
        rules["bb.cnx.%d.W1" % i] = rules["bb.cnx.%d.W2" % i] = (0, 1)
    if "sd.first.w" in names:
        rules["sd.first.w"] = rules["sd.lstm.Wih0"] = (0, 1)
        cin = NF << len(arch.ratios)
        for i, _r in enumerate(arch.ratios):
            s, h = "sd.stage%d" % (i + 1), cin // 2
            rules[s + ".tr_wp"] = (0, 1)
            if not fusable(h):
                for c in (".sc.w", ".c3.w", ".c1.w", ".cat.w"):
                    rules[s + c] = (0, 1)
            cin = h
    return rules


def copy_name(name):
    return name[:-2] + ".s32" if name.endswith(".w") else name + ".s32"


class Entry:
    """One array as loaded: what wt_model_weight_info says and the words themselves (fp32 array in its dims, or uint16 flat)."""
    def __init__(self, name, data, fmt=F32, of="", acc_scale=1.0, tap_pair=0, lazy=0, lazy_scale=1.0):
        self.name, self.data, self.fmt, self.of = name, data, fmt, of
        self.acc_scale, self.tap_pair, self.lazy, self.lazy_scale = float(acc_scale), int(tap_pair), int(lazy), float(lazy_scale)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def check_copy(e, w, stride):
    """The S32 copy e of the loaded fp32 array w: acc_scale = 1 / s32_weight_scale(amax) and every word the emulation's of w s
    (taps in paired order for stride > 0); returns worst |w - value acc_scale| / bound over the elements the bound covers."""
    w = np.asarray(w, np.float32)
    if e.name == "vq.embed.s32":
        w = w[0]
    amax = float(np.abs(w).max())
    s = f16_ref.s32_weight_scale(amax)
    assert s != 0.0 and np.isfinite(w).all(), (e.name, "no split form: amax %g" % amax)
    assert e.acc_scale == 1.0 / s, (e.name, "acc_scale %g, expected %g (amax %g)" % (e.acc_scale, 1.0 / s, amax))
    assert e.tap_pair == (1 if stride else 0), (e.name, "tap_pair flag")
    if stride:
        w = w[:, tap_pair_order(w.shape[1], stride), :]
    v = (w * np.float32(s)).reshape(-1)
    assert same_words(e.data, split_emulate(v), s32=True), (e.name, "S32 words differ from the split of the loaded fp32 array times %g" % s)
    err = np.abs(v.astype(np.float64) - split_value(e.data)) / split_bound(v)
    assert float(err.max()) <= 1.0, (e.name, "split bound", float(err.max()))
    return float(err.max())


_EXPECTED = {}


def check_model(arch, sd, entries):
    """entries: [Entry] of a model loaded from sd.  Every entry is compared, every expected array must be there; raises
    AssertionError naming the first array that is wrong.  Returns {class: worst err / bound} and the count of fold words
    that differ from the reference rounded to fp32, as {"fold_words": (different, all)}."""
    if _EXPECTED.get("key") != (id(arch), id(sd)):         # the last one, kept with its state dict: computed once per model
        _EXPECTED.update(key=(id(arch), id(sd)), sd=sd, arch=arch, exp=expected(arch, sd))
    exp = _EXPECTED["exp"]
    by = {e.name: e for e in entries}
    assert len(by) == len(entries), "duplicate names"
    get = lambda n: np.asarray(by[n].data)
    rules = copy_rules(arch, set(by))
    want = set(exp) | {copy_name(n) for n in rules}
    assert set(by) == want, ("arrays missing / unknown", sorted(want - set(by))[:5], sorted(set(by) - want)[:5])
    stats, diff, total = {}, 0, 0
    worst = lambda c, v: stats.__setitem__(c, max(stats.get(c, 0.0), v))
    for name, r in exp.items():
        e = by[name]
        assert e.fmt == r.fmt, (name, "format", e.fmt)
        rule = rules.get(name)
        assert e.lazy == (2 if name.endswith(".wpair") else rule[1] if rule else 0), (name, "lazy flag", e.lazy)
        if r.kind == "bound":
            got = np.asarray(e.data, np.float64)
            assert got.shape == r.ref.shape, (name, got.shape, r.ref.shape)
            zero = r.bound == 0
            assert np.all(bits32(e.data)[zero.reshape(-1)] == 0) if r.cls == "basis" else np.all(got[zero] == r.ref[zero]), (name, "entries that must be exactly 0")
            with np.errstate(divide="ignore", invalid="ignore"):
                err = np.where(zero, 0.0, np.abs(got - r.ref) / r.bound)
            assert np.isfinite(got).all() and float(err.max()) <= 1.0, (name, "worst err / bound", float(err.max()))
            worst(r.cls, float(err.max()))
            if r.cls == "fold":
                diff += int((bits32(e.data) != bits32(r.ref.astype(np.float32))).sum())
                total += got.size
        else:
            ref = r.fn(get) if r.kind == "derived" else r.ref
            got = np.asarray(e.data).reshape(-1)
            ref = np.ascontiguousarray(ref).reshape(-1)
            assert got.shape == ref.shape and (got.dtype == np.uint16) == (ref.dtype == np.uint16), (name, got.shape, ref.shape)
            same = same_words(got, ref) if ref.dtype == np.uint16 else bool(np.array_equal(bits32(got), bits32(ref)))
            assert same, (name, "not bit-identical to the rearranged raw tensors")
            worst(r.cls, 0.0)
    for name, (stride, lazy) in rules.items():
        e = by[copy_name(name)]
        assert e.fmt == S32 and e.of == name, (e.name, "format / of", e.fmt, e.of)
        worst("split", check_copy(e, get(name), stride))
        if lazy:
            assert by[name].lazy_scale * e.acc_scale == 1.0, (name, "LazyF32::scale and acc_scale", by[name].lazy_scale, e.acc_scale)
    stats["fold_words"] = (diff, total)
    return stats


def check_packed(orig, packed):
    """packed: the entries of the model made from orig's packed image.  Stored arrays bit-identical, rebuilt ones within
    max(2^-22 |w|, 2^-36 acc_scale), the two scales consistent.  Returns the worst rebuilt err / bound."""
    a, b = {e.name: e for e in orig}, {e.name: e for e in packed}
    assert set(a) == set(b), sorted(set(a) ^ set(b))[:5]
    worst = 0.0
    for name, e in a.items():
        p = b[name]
        assert (p.fmt, p.of, p.acc_scale, p.tap_pair, p.lazy, p.lazy_scale) == (e.fmt, e.of, e.acc_scale, e.tap_pair, e.lazy, e.lazy_scale), (name, "record")
        if e.lazy == 2:
            continue                     # nothing reads it after the load: a packed model holds no defined values there
        if e.lazy == 0:
            assert np.array_equal(np.ascontiguousarray(p.data).view(np.uint8), np.ascontiguousarray(e.data).view(np.uint8)), (name, "stored array differs")
            continue
        acc = a[copy_name(name)].acc_scale
        assert e.lazy_scale * acc == 1.0, (name, "scales")
        w = np.asarray(e.data, np.float64)
        err = np.abs(np.asarray(p.data, np.float64) - w) / np.maximum(2.0 ** -22 * np.abs(w), 2.0 ** -36 * acc)
        assert float(err.max()) <= 1.0, (name, "rebuilt array: worst err / bound", float(err.max()))
        worst = max(worst, float(err.max()))
    return worst
