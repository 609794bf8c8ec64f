"""CPU-only half of tests/test_model_weights.py: tests/weights_ref.py's checker passes an honest numpy evaluation of every
load-time transform of weights.cpp (double arithmetic and one cast where the library does that, fp32 where it does that) and
fails each of the slips it is there for; the split emulation meets its bound with equality at most; s32_weight_scale's
contract on the CPU mirror."""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from tests import enc_ref, f16_ref, weights_ref as W

# slip -> (the array the checker must name, what it must say about it)
SLIPS = {"tr_norm_axis": ("sd.stage1.tr_w", "worst err / bound"), "tap_pair_order": ("enc.stage1.down.wpair", "not bit-identical"),
         "cat_bias": ("enc.stage3.cat.b", "not bit-identical"), "k_before_q": ("bb.attn.Wqk", "not bit-identical"),
         "head_swap": ("head.W", "not bit-identical"), "nyquist_sine": ("istft.W", "exactly 0"), "ce_for_odd": ("istft.W", "worst err / bound"),
         "lo_2_10": ("enc.stage1.down.s32", "S32 words differ"), "lo_in_hi_slot": ("enc.stage1.down.s32", "S32 words differ"),
         "acc_scale_x2": ("enc.stage1.down.s32", "acc_scale 2, expected 1"), "scale_wrong_tensor": ("istft.W.s32", "acc_scale 1, expected"),
         "ee_book1": ("vq.ee", "worst err / bound")}


@functools.lru_cache(maxsize=None)
def _case():
    """A two-block, two-codebook hop320 model with the SEANetDecoder: every transform of the full models, a tenth of the words.
    istft.W is the one tensor of the synthetic recipe outside the scale window; the codebook is moved above it and W2 of
    block 0 below it, so that the scaled route is there for three kinds of tensor."""
    from wavtokenizer_amd import synth
    from wavtokenizer_amd.config import NAMED_ARCHS
    arch = dataclasses.replace(NAMED_ARCHS["hop320"], num_layers=2, num_quantizers=2)
    sd = dict(synth.make_state_dict(arch, seed=3, with_seanet_decoder=True))
    sd[(W.VQ % 0) + "embed"] = sd[(W.VQ % 0) + "embed"] * np.float32(2.0 ** 14)
    sd["backbone.convnext.0.pwconv2.weight"] = sd["backbone.convnext.0.pwconv2.weight"] * np.float32(2.0 ** -20)
    return arch, sd


def _fold(g, v, per_dim1=False):
    """fold_wn of weights.cpp: double arithmetic, one cast."""
    v64 = np.asarray(v, np.float64)
    g64 = np.asarray(g, np.float64).reshape(-1)
    if per_dim1:             # the slip: the norm over (cin, k) per cout, as for an ordinary conv, with g still per cin
        ss = (v64 ** 2).sum(axis=(0, 2))
        return (g64[:, None, None] / np.sqrt(ss)[None, :, None] * v64).astype(np.float32)
    ss = (v64.reshape(v64.shape[0], -1) ** 2).sum(1)
    return ((g64 / np.sqrt(ss)).reshape((-1,) + (1,) * (v64.ndim - 1)) * v64).astype(np.float32)


def _split(v, slip):
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(1024.0 if slip == "lo_2_10" else 2048.0)).astype(np.float16)
    pair = [lo, hi] if slip == "lo_in_hi_slot" else [hi, lo]
    return np.stack([p.reshape(-1, 32) for p in pair], 1).reshape(-1).view(np.uint16)


def load_emulation(arch, sd, slip=None):
    """[W.Entry] of wt_model_create on (arch, sd), in numpy: build_model, then build_splits."""
    E = {}
    put = lambda name, a, **kw: E.__setitem__(name, W.Entry(name, np.ascontiguousarray(a), **kw))
    D, N = arch.dim, arch.n_fft

    def wn(prefix, name):
        put(name + ".w", _fold(sd[prefix + ".weight_g"], sd[prefix + ".weight_v"]).transpose(0, 2, 1))
        put(name + ".b", sd[prefix + ".bias"])

    def plain(prefix, name):
        put(name + ".w", np.asarray(sd[prefix + ".weight"], np.float32).transpose(0, 2, 1))
        put(name + ".b", sd[prefix + ".bias"])

    def lstm(prefix, name):
        k = lambda s: sd[prefix + ".lstm." + s]
        p = W.lstm_packings(k("weight_ih_l0"), k("weight_hh_l0"), k("weight_ih_l1"), k("weight_hh_l1"),
                            k("bias_ih_l0"), k("bias_hh_l0"), k("bias_ih_l1"), k("bias_hh_l1"))
        for s, a in p.items():
            put(name + "." + s, a, fmt={"W0h": W.LSTM_F16, "W1h": W.LSTM_F16, "Wp": W.LSTM_PERSIST}.get(s, W.F32))

    def cat(p, s):
        put(s + ".cat.w", np.concatenate([E[s + ".sc.w"].data[:, 0, :], E[s + ".c1.w"].data[:, 0, :]], 1)[:, None, :])
        b1 = np.asarray(sd[p + ".block.3.conv.conv.bias"], np.float32)
        put(s + ".cat.b", b1 if slip == "cat_bias" else np.asarray(sd[p + ".shortcut.conv.conv.bias"], np.float32) + b1)

    put("enc.e0.w", _fold(sd[W.ENC + "0.conv.conv.weight_g"], sd[W.ENC + "0.conv.conv.weight_v"])[:, 0, :].T)
    put("enc.e0.b", sd[W.ENC + "0.conv.conv.bias"])
    idx, C = 1, W.NF
    for i, r in enumerate(arch.enc_ratios):
        p, s = W.ENC + str(idx), "enc.stage%d" % (i + 1)
        wn(p + ".block.1.conv.conv", s + ".c3")
        wn(p + ".block.3.conv.conv", s + ".c1")
        wn(p + ".shortcut.conv.conv", s + ".sc")
        wn(W.ENC + "%d.conv.conv" % (idx + 2), s + ".down")
        order = [(q >> 1) + (q & 1) * r for q in range(2 * r)]
        if slip == "tap_pair_order":
            order = [(q >> 1) + (1 - (q & 1)) * r for q in range(2 * r)]             # (r, 0, r + 1, 1, ...)
        put(s + ".down.wpair", E[s + ".down.w"].data[:, order, :], lazy=2)
        if not W.fusable(C):
            cat(p, s)
        idx, C = idx + 3, 2 * C
    lstm(W.ENC + str(idx), "enc.lstm")
    wn(W.ENC + "%d.conv.conv" % (idx + 2), "enc.final")
    books = [np.asarray(sd[(W.VQ % q) + "embed"], np.float32) for q in range(arch.num_quantizers)]
    put("vq.embed", np.stack(books, 0))
    e = books[1 if slip == "ee_book1" else 0]
    acc = np.zeros(e.shape[0], np.float32)
    for c in range(e.shape[1]):                                   # the fp32 running sum
        acc = acc + e[:, c] * e[:, c]
    put("vq.ee", acc)
    plain("backbone.embed", "bb.embed")
    for i, ri in enumerate((0, 1, 3, 4)):
        p, s = "backbone.pos_net.%d" % ri, "bb.res.%d" % i
        for a, b in (("n1w", "norm1.weight"), ("n1b", "norm1.bias"), ("n2w", "norm2.weight"), ("n2b", "norm2.bias")):
            put(s + "." + a, sd[p + "." + b])
        plain(p + ".conv1", s + ".c1")
        plain(p + ".conv2", s + ".c2")
    p = "backbone.pos_net.2."
    flat = lambda k: np.asarray(sd[k], np.float32).reshape(D, D)
    qk = ["k", "q"] if slip == "k_before_q" else ["q", "k"]
    put("bb.attn.nw", sd[p + "norm.weight"]), put("bb.attn.nb", sd[p + "norm.bias"])
    put("bb.attn.Wqk", np.concatenate([flat(p + t + ".weight") for t in qk], 0))
    put("bb.attn.bqk", np.concatenate([sd[p + t + ".bias"] for t in qk]))
    put("bb.attn.Wv", flat(p + "v.weight")), put("bb.attn.bv", sd[p + "v.bias"])
    put("bb.attn.Wp", flat(p + "proj_out.weight")), put("bb.attn.bp", sd[p + "proj_out.bias"])
    put("bb.gn5.w", sd["backbone.pos_net.5.weight"]), put("bb.gn5.b", sd["backbone.pos_net.5.bias"])
    put("bb.ada.s", sd["backbone.norm.scale.weight"]), put("bb.ada.h", sd["backbone.norm.shift.weight"])
    for i in range(arch.num_layers):
        p, s = "backbone.convnext.%d." % i, "bb.cnx.%d." % i
        put(s + "dw_w", np.asarray(sd[p + "dwconv.weight"], np.float32).reshape(D, 7).T)
        for a, b in (("dw_b", "dwconv.bias"), ("ada_s", "norm.scale.weight"), ("ada_h", "norm.shift.weight"), ("W1", "pwconv1.weight"),
                     ("b1", "pwconv1.bias"), ("W2", "pwconv2.weight"), ("b2", "pwconv2.bias"), ("gamma", "gamma")):
            put(s + a, sd[p + b])
    put("bb.fln.w", sd["backbone.final_layer_norm.weight"]), put("bb.fln.b", sd["backbone.final_layer_norm.bias"])
    # the head: 32-row groups, 16 log-magnitude rows then the 16 phase rows of the same slots
    Kq, Kb, bins = W.head_slots(N)
    nb = N // 2 + 1
    w, b = np.asarray(sd["head.out.weight"], np.float32).reshape(N + 2, D), np.asarray(sd["head.out.bias"], np.float32)
    hw, hb = np.zeros((2 * Kb, D), np.float32), np.zeros(2 * Kb, np.float32)
    for sl, f in enumerate(bins):
        if f < 0:
            continue
        pm = (sl // 16) * 32 + sl % 16
        pp = pm + 16
        if slip == "head_swap":
            pm, pp = pp, pm
        hw[pm], hw[pp], hb[pm], hb[pp] = w[f], w[nb + f], b[f], b[nb + f]
    put("head.W", hw), put("head.b", hb)
    Q = N // 4
    basis = np.zeros((4, Kq, Kq), np.float32)
    for n in range(Q + 1):
        g = np.arange(Q + 1)
        fe, fo = 2 * g, 2 * g + 1
        edge = (fe == 0) | (fe == N // 2)
        ce, co = np.where(edge, 1.0, 2.0) / N, 2.0 / N
        the = 2.0 * math.pi * ((fe * n) % N) / N
        tho = 2.0 * math.pi * ((fo * n) % N) / N
        basis[0, n, :Q + 1] = ce * np.cos(the)
        basis[2, n, :Q + 1] = ce * np.sin(the) if slip == "nyquist_sine" else np.where(edge, 0.0, ce * np.sin(the))
        basis[1, n, :Q] = ((ce if slip == "ce_for_odd" else co) * np.cos(tho))[:Q]
        basis[3, n, :Q] = ((ce if slip == "ce_for_odd" else co) * np.sin(tho))[:Q]
    put("istft.W", basis)
    win = np.asarray(sd["head.istft.window"], np.float32)
    put("istft.win", win), put("istft.wsq", win * win)
    if W.DEC + "0.conv.conv.weight_v" in sd:
        wn(W.DEC + "0.conv.conv", "sd.first")
        lstm(W.DEC + "1", "sd.lstm")
        di, cin = 2, W.NF << len(arch.ratios)
        for i, r in enumerate(arch.ratios):
            p, s = W.DEC + "%d.convtr.convtr" % (di + 1), "sd.stage%d" % (i + 1)
            wf = _fold(sd[p + ".weight_g"], sd[p + ".weight_v"], per_dim1=(slip == "tr_norm_axis"))       # [cin][cout][k]
            put(s + ".tr_w", wf.transpose(2, 0, 1))
            pp = np.empty((r, wf.shape[1], 2, wf.shape[0]), np.float32)
            for ph in range(r):
                pp[ph, :, 0, :] = wf[:, :, ph + r].T
                pp[ph, :, 1, :] = wf[:, :, ph].T
            put(s + ".tr_wp", pp)
            put(s + ".tr_b", sd[p + ".bias"])
            rp, h = W.DEC + str(di + 2), cin // 2
            wn(rp + ".block.1.conv.conv", s + ".c3")
            wn(rp + ".block.3.conv.conv", s + ".c1")
            wn(rp + ".shortcut.conv.conv", s + ".sc")
            if not W.fusable(h):
                cat(rp, s)
            di, cin = di + 3, h
        p = W.DEC + "%d.conv.conv" % (di + 1)
        put("sd.last.w", _fold(sd[p + ".weight_g"], sd[p + ".weight_v"])[0].T)
        put("sd.last.b", sd[p + ".bias"])
    # build_splits
    for name, (stride, lazy) in W.copy_rules(arch, set(E)).items():
        src = E[name + "pair" if stride else name].data
        if name == "vq.embed":
            src = src[0]
        amax_of = E["head.W"].data if (slip == "scale_wrong_tensor" and name == "istft.W") else src
        s = f16_ref.s32_weight_scale(float(np.abs(amax_of).max()))
        acc = 1.0 / s
        put(W.copy_name(name), _split(src * np.float32(s), slip), fmt=W.S32, of=name, acc_scale=acc * (2.0 if slip == "acc_scale_x2" else 1.0),
            tap_pair=1 if stride else 0)
        if lazy:
            E[name].lazy, E[name].lazy_scale = 1, s
    return list(E.values())


def packed_emulation(entries, slip=None):
    """The entries of the model that wt_model_create_packed makes from the image of `entries`, after ensure_f32_weights."""
    by = {e.name: e for e in entries}
    out = []
    for e in entries:
        d = e.data
        if e.lazy == 1:
            c = by[W.copy_name(e.name)]
            d = np.zeros_like(e.data) if slip == "lazy_unrebuilt" else W.split_value_f32(c.data, 1.0 / e.lazy_scale).reshape(e.data.shape)
        elif e.lazy == 2:
            d = np.zeros_like(e.data)
        out.append(W.Entry(e.name, d, e.fmt, e.of, e.acc_scale, e.tap_pair, e.lazy, e.lazy_scale))
    return out


@functools.lru_cache(maxsize=None)
def _honest():
    arch, sd = _case()
    return load_emulation(arch, sd)


def test_checker_accepts_an_honest_load():
    arch, sd = _case()
    stats = W.check_model(arch, sd, _honest())
    print(stats)
    by = {e.name: e for e in _honest()}
    scaled = [n for n, e in by.items() if e.fmt == W.S32 and e.acc_scale != 1.0]
    assert sorted(scaled) == ["bb.cnx.0.W2.s32", "istft.W.s32", "vq.embed.s32"], scaled
    assert by["vq.embed.s32"].acc_scale > 1 > by["bb.cnx.0.W2.s32"].acc_scale
    diff, total = stats["fold_words"]
    assert diff <= total * 1e-6, (diff, total)          # a double-rounding case is rarer than 2^-29 per word
    for cls in ("fold", "ee", "basis", "split"):
        assert 0 < stats[cls] <= 1.0, (cls, stats[cls])


@pytest.mark.parametrize("slip", SLIPS)
def test_checker_rejects_each_slip(slip):
    arch, sd = _case()
    name, what = SLIPS[slip]
    with pytest.raises(AssertionError) as ei:
        W.check_model(arch, sd, load_emulation(arch, sd, slip))
    print(slip, "->", str(ei.value)[:160])
    assert ei.value.args[0][0] == name and what in ei.value.args[0][1], ei.value.args


def test_checker_of_a_packed_round_trip():
    worst = W.check_packed(_honest(), packed_emulation(_honest()))
    assert 0 < worst <= 1.0
    with pytest.raises(AssertionError, match="rebuilt"):
        W.check_packed(_honest(), packed_emulation(_honest(), "lazy_unrebuilt"))


def test_fold_reference_agrees_with_the_float64_one():
    """weights_ref.fold_ref (norm in long double) rounds to enc_ref.fold_weight_norm's fp32 values except in double-rounding cases."""
    arch, sd = _case()
    p = W.ENC + "3.conv.conv"
    ref, bound = W.fold_ref(sd[p + ".weight_g"], sd[p + ".weight_v"])
    old = enc_ref.fold_weight_norm(sd[p + ".weight_g"], sd[p + ".weight_v"]).numpy()
    assert np.all(np.abs(old - ref) <= bound)
    assert (old.astype(np.float32) != ref.astype(np.float32)).mean() < 1e-5


def test_dft_reference_agrees_with_the_full_basis():
    """The quarter bases are rows of f16_ref.istft_basis (no window): even / odd bins, n <= N / 4.  That one takes the cosine of
    the unreduced angle in float64, so the agreement is to 1e-9 of the largest entry only."""
    for N in (1280, 2400):
        ref, bound = W.dft_basis(N)
        Q, nb = N // 4, N // 2 + 1
        full = f16_ref.istft_basis(N, torch.ones(N)).numpy()
        tol = 1e-9 * 2.0 / N
        assert np.abs(ref[0, :Q + 1, :Q + 1] - full[0:nb:2, :Q + 1].T).max() < tol
        assert np.abs(ref[1, :Q + 1, :Q] - full[1:nb:2, :Q + 1].T).max() < tol
        assert np.abs(ref[2, :Q + 1, :Q + 1] + full[nb:2 * nb:2, :Q + 1].T).max() < tol
        assert np.abs(ref[3, :Q + 1, :Q] + full[nb + 1:2 * nb:2, :Q + 1].T).max() < tol
        assert np.all(ref[2, :, 0] == 0) and np.all(ref[2, :, Q] == 0) and np.all(bound[2, :, 0] == 0) and np.all(bound[2, :, Q] == 0)
        assert np.all(ref[:, Q + 1:, :] == 0) and np.all(ref[:, :, Q + 1:] == 0) and np.all(ref[[1, 3], :, Q] == 0)


def test_split_emulation_meets_its_bound():
    """|v - (hi + lo 2^-11)| <= max(2^-22 |v|, 2^-36) on log-uniform fp32 values, ties, f16 subnormals and signed zeros, with
    equality somewhere (so the comparison is <=), and the fp32 evaluation hi + lo / 2048 is the float64 one exactly."""
    rng = np.random.default_rng(0)
    n = 1 << 22
    v = (np.exp2(rng.uniform(-40, 15.99, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    edge = np.array([0.0, -0.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65503.9, 2.0 ** -36,
                     2.0 ** -37, 3 * 2.0 ** -37, 2.0 ** -24 + 2.0 ** -36, 1 + 2.0 ** -11 + 2.0 ** -22, 0.1, -0.1], np.float32)
    v[:edge.size] = edge
    words = W.split_emulate(v)
    val = W.split_value(words)
    err = np.abs(v.astype(np.float64) - val) / W.split_bound(v)
    assert err.max() <= 1.0, err.max()
    assert err.max() == 1.0                                   # 2^-36: hi = 0, lo = f16(2^-25) ties to 0: the bound is met with equality
    assert np.array_equal(W.split_value_f32(words).astype(np.float64), val)
    hi, lo = W.split_halves(words)
    assert hi[0] == 0 and not np.signbit(hi[0]) and np.signbit(hi[1]) and lo[4] == np.float16(2.0 ** -14) and hi[4] == 0
    # layout: element i at g = (i >> 5) * 64 + (i & 31), lo at g + 32
    i = np.arange(96)
    g = (i >> 5) * 64 + (i & 31)
    w96 = W.split_emulate(np.arange(1, 97, dtype=np.float32) + np.float32(0.25 * 2.0 ** -11))
    assert np.array_equal(w96.view(np.float16)[g], np.arange(1, 97, dtype=np.float16))
    assert np.array_equal(w96.view(np.float16)[g + 32], np.full(96, 0.25, np.float16))


def test_s32_weight_scale_contract():
    """acc_scale = 1 / scale is 1 on [2^-6, 2^12) and at 0; elsewhere scale and acc_scale are finite, positive, normal powers of
    two.  Below the window amax * scale lies in [1, 2).  Above it amax * scale lies in [2^11, 2^12), the window's top binade, not in
    [1, 2): the split form's floor is absolute (2^-36), so every binade the maximum is lowered by takes a bit from the tensor's
    small elements, and the plans on a conv weight with one planted 2^13 (tests/test_model_weights.py, conv2) were 6.4 times the
    fp32 reference's distance from float64 with [1, 2), against a bar of 4.  Below 2^-126 no pair of normal floats (scale,
    1 / scale) brings the maximum into [1, 2) (it needs scale > 2^126) and the answer is 0: the tensor is not split."""
    S = f16_ref.s32_weight_scale
    nx = lambda x, d: float(np.nextafter(np.float32(x), np.float32(d)))
    for a in (0.0, 2.0 ** -6, nx(2.0 ** 12, 0), 1.0, 0.3, 100.0):
        assert S(a) == 1.0, a
    rng = np.random.default_rng(1)
    fmax = float(np.finfo(np.float32).max)
    grid = [nx(2.0 ** -6, 0), 2.0 ** 12, 2.0 ** -126, nx(2.0 ** 127, 0), 2.0 ** 126, 2.0 ** 127, 3e38, fmax, 2.0 ** -100, 2.0 ** 100, 1e-30, 3e30]
    grid += list(np.exp2(rng.uniform(-126, -6, 200)).astype(np.float32)) + list(np.exp2(rng.uniform(12, 127.99, 200)).astype(np.float32))
    tiny = float(np.finfo(np.float32).tiny)
    for a in grid:
        a = float(np.float32(a))
        if 2.0 ** -6 <= a < 2.0 ** 12:
            continue
        s = S(a)
        acc = 1.0 / s
        for x in (s, acc):
            assert np.float32(x) == x and tiny <= x < float("inf") and math.frexp(x)[0] == 0.5, (a, x)
        if a < 1.0:
            assert 1.0 <= a * s < 2.0, (a, s)
        else:
            assert 2.0 ** 11 <= a * s < 2.0 ** 12, (a, s)
    for a in (nx(2.0 ** -126, 0), 2.0 ** -127, 2.0 ** -128, 1e-40, float(np.float32(1e-45)), float("inf")):
        assert S(a) == 0.0, a
