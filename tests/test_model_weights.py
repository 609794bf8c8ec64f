"""GPU: what wt_model_create leaves in HBM, array by array (wt_model_weight_info), against tests/weights_ref.py; the same model
through its packed image; the edges of the S32 copies' scale window on one GEMM weight; and the plans on scaled copies
against the float64 oracle.  The CPU half (the checker's own tests) is tests/test_weight_checks.py."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import f16_ref, range_ref, weights_ref as W
from tests.range_ref import BW
from tests.util import check_codes, manifest, rel_l2, synth_state_dict

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _hip():
    lib = ctypes.CDLL("libamdhip64.so")
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return lib


def _read(ptr, words):
    torch.cuda.synchronize()
    host = np.empty(words, np.uint32)
    assert _hip().hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), words * 4, 2) == 0      # device to host
    return host


def _infos(model):
    from wavtokenizer_amd._capi import lib, check, WtWeightInfo
    out = []
    for i in range(lib.wt_model_weight_count(model)):
        w = WtWeightInfo(size=ctypes.sizeof(WtWeightInfo))
        check(lib.wt_model_weight_info(model, i, ctypes.byref(w)), "wt_model_weight_info")
        out.append(w)
    return out


def _entry(w):
    raw = _read(w.data, w.numel)
    if w.format == W.F32:
        data = raw.view(np.float32).reshape([w.dims[i] for i in range(w.ndim)])
    else:
        data = raw.view(np.uint16)
    return W.Entry(w.name.decode(), data, w.format, w.of.decode(), w.acc_scale, w.tap_pair, w.lazy, w.lazy_scale)


def _entries(model, names=None):
    return [_entry(w) for w in _infos(model) if names is None or w.name.decode() in names]


def _engine(arch, sd):
    from wavtokenizer_amd.pretrained import _Engine
    e = _Engine()
    e.load(arch, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, torch.cuda.current_device())
    return e


def _fresh(arch, sd):
    from wavtokenizer_amd import WavTokenizer
    m = WavTokenizer.from_arch(arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    m = m.eval().to("cuda")
    m._ensure_engine()
    return m


def _quiet(m):
    m.check_status()
    assert not m.fallback_events


def _allocations(image):
    """[(bytes, stored)] of the model's allocations, from the table at the head of its packed image (weights.cpp PackHeader)."""
    from wavtokenizer_amd._capi import WtArch

    class _PackHeader(ctypes.Structure):
        _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_int32), ("arch", WtArch), ("arch_hash", ctypes.c_uint64),
                    ("n_allocs", ctypes.c_uint64), ("struct_bytes", ctypes.c_uint64), ("payload_bytes", ctypes.c_uint64), ("body_hash", ctypes.c_uint64)]

    h = _PackHeader.from_buffer_copy(image[:ctypes.sizeof(_PackHeader)].tobytes())
    assert h.magic == 0x4b505457
    t = image[ctypes.sizeof(_PackHeader):ctypes.sizeof(_PackHeader) + 8 * h.n_allocs].view(np.uint64)
    return [(int(b & ~np.uint64(1 << 63)), not bool(b >> np.uint64(63))) for b in t]


def _variant(which):
    from wavtokenizer_amd import NAMED_ARCHS, synth
    if which in ("hop600", "hop320"):
        return NAMED_ARCHS[which], synth_state_dict(which)
    if which == "hop600+seanet":
        return NAMED_ARCHS["hop600"], synth.make_state_dict(NAMED_ARCHS["hop600"], seed=manifest()["weight_seed"], with_seanet_decoder=True)
    arch = dataclasses.replace(NAMED_ARCHS["hop600"], num_quantizers=3)            # the three-codebook fixture's architecture
    return arch, synth.make_state_dict(arch, seed=manifest()["weight_seed"])


# ------------------------------------------------------------------------------------------------ every array
@gpu
@pytest.mark.parametrize("which", ["hop600", "hop320", "hop600+seanet", "hop600x3"])
def test_every_loaded_array(which):
    """Every array the enumerator names is compared (weights_ref.check_model: fp32 arrays bit-exact or within the derived bound,
    S32 copies against the emulation of their own fp32 array times the scale, acc_scale = 1 / s32_weight_scale(amax), tap_pair
    exactly on the down convs); every allocation of the model is named by exactly one entry; archive_model writes the same set
    of pointers.  Then the model made from the packed image: stored arrays bit-identical, rebuilt ones within
    max(2^-22 |w|, 2^-36 acc_scale).  Zero arrays skipped."""
    arch, sd = _variant(which)
    eng = _engine(arch, sd)
    infos = _infos(eng.model)
    ents = [_entry(w) for w in infos]
    stats = W.check_model(arch, sd, ents)
    print(f"loaded arrays {which}: {len(ents)} arrays, worst err / bound per class {stats}")
    for e in ents:
        if e.fmt == W.S32 and e.acc_scale != 1.0:
            print(f"  scaled copy {e.name}: acc_scale {e.acc_scale:g}")
    assert all(w.archived for w in infos), [w.name for w in infos if not w.archived][:5]
    ptrs = [w.data for w in infos]
    assert len(set(ptrs)) == len(ptrs), "two names for one array"
    image = eng.export()
    allocs = _allocations(image)
    # pointers, not sizes: every allocation of the image's table is the base of exactly one entry, and every entry is one.
    # An upload holds max(words, 4) words; an S32 copy the words of its fp32 array; the arrays a packed image leaves out are
    # exactly the lazy ones
    assert sorted(w.alloc for w in infos) == list(range(len(allocs))), ("allocations that no entry starts at, or entries that are no allocation",
                                                                        sorted(set(range(len(allocs))) - {w.alloc for w in infos})[:6], [w.name for w in infos if w.alloc < 0][:6])
    for w in infos:
        assert allocs[w.alloc] == (max(w.numel, 4) * 4, w.lazy == 0), (w.name, allocs[w.alloc], w.numel, w.lazy)
    from wavtokenizer_amd.pretrained import _Engine
    pk = _Engine()
    pk.load_packed(image, torch.cuda.current_device())
    pinfos = _infos(pk.model)
    assert [w.name for w in pinfos] == [w.name for w in infos]
    worst = W.check_packed(ents, [_entry(w) for w in pinfos])
    print(f"packed round trip {which}: rebuilt fp32 arrays worst err / bound {worst:.4f}")
    assert _allocations(pk.export()) == allocs
    pk.close()
    eng.close()


# ------------------------------------------------------------------------------------------------ window edges
KEY = "backbone.convnext.0.pwconv1.weight"
NX = lambda x, d: float(np.nextafter(np.float32(x), np.float32(d)))
EDGE_AMAX = {"2^-6": 2.0 ** -6, "below 2^-6": NX(2.0 ** -6, 0), "below 2^12": NX(2.0 ** 12, 0), "2^12": 2.0 ** 12, "2^-126": 2.0 ** -126,
             "2^-127": 2.0 ** -127, "2^-128": 2.0 ** -128, "1e-40": 1e-40, "2^126": 2.0 ** 126, "2^127": 2.0 ** 127, "3e38": 3e38}
DEAD = 5


def _edge_dict(amax):
    """hop320's synthetic weights with pwconv1.weight of block 0 at the given maximum.  Below the window the whole tensor is
    scaled by a power of two and its largest element set to the value; above it one element is planted in column DEAD, whose
    operand (the block's AdaNorm output) is made exactly zero through the scale and shift tables."""
    sd = dict(synth_state_dict("hop320"))
    w = sd[KEY].copy()
    a0 = float(np.abs(w).max())
    at = np.unravel_index(int(np.abs(w).argmax()), w.shape)
    if amax < 1.0:
        k = int(np.floor(np.log2(amax / a0)))
        with np.errstate(under="ignore"):
            w = w * np.float32(2.0 ** k) if k >= -126 else (w * np.float32(2.0 ** -100)) * np.float32(2.0 ** (k + 100))
        assert float(np.abs(w).max()) <= amax
        w[at] = np.float32(amax)
    else:
        for t in ("scale", "shift"):
            v = sd["backbone.convnext.0.norm.%s.weight" % t].copy()
            v[:, DEAD] = 0.0
            sd["backbone.convnext.0.norm.%s.weight" % t] = v
        w[7, DEAD] = np.float32(amax)
    assert float(np.abs(w).max()) == float(np.float32(amax))
    sd[KEY] = w
    return sd


@gpu
@pytest.mark.parametrize("case", list(EDGE_AMAX))
def test_scale_window_edges(case):
    """One of two things holds at every maximum: the copy and acc_scale are exact by check_copy's rules with every word finite,
    or wt_model_split_ok is 0 and the plans run on the fp32 chain (the default decode plan's output is the FP32_GEMM plan's, bit
    for bit).  Never a non-finite copy with s32_ok set.  The maxima below 2^-126 are the second kind: no pair of normal floats
    (scale, 1 / scale) brings them into [1, 2).  Those from 2^127 on are the first: 2^(12 - e) and its reciprocal are normal."""
    from wavtokenizer_amd import NAMED_ARCHS, _capi
    arch = NAMED_ARCHS["hop320"]
    amax = float(np.float32(EDGE_AMAX[case]))
    sd = _edge_dict(amax)
    m = _fresh(arch, sd)
    model = m._engine.model
    by = {e.name: e for e in _entries(model, {"bb.cnx.0.W1", "bb.cnx.0.W1.s32"})}
    w, c = by["bb.cnx.0.W1"], by["bb.cnx.0.W1.s32"]
    assert np.array_equal(W.bits32(w.data), W.bits32(sd[KEY])), "the loaded fp32 array is not the state dict's"
    ok = _capi.lib.wt_model_split_ok(model)
    hi, lo = W.split_halves(c.data)
    finite = bool(np.isfinite(hi).all() and np.isfinite(lo).all())
    want = f16_ref.s32_weight_scale(amax)
    print(f"window edge {case}: amax {amax:g}, split_ok {ok}, acc_scale {c.acc_scale:g}, lazy_scale {w.lazy_scale:g}, copy finite {finite}")
    assert np.isfinite(c.acc_scale) and c.acc_scale > 0 and np.isfinite(w.lazy_scale) and w.lazy_scale > 0
    assert ok or not w.lazy, "an array whose copy is unusable must stay stored"
    if ok:
        assert want != 0.0 and finite
        W.check_copy(c, w.data, 0)
        assert (c.acc_scale == 1.0) == (2.0 ** -6 <= amax < 2.0 ** 12)
        assert w.lazy == 1 and w.lazy_scale * c.acc_scale == 1.0
    else:
        assert want == 0.0, "the split was given up inside the range that has a scale"
        feats = range_ref.features(1, 20).cuda()
        dev = torch.device("cuda", torch.cuda.current_device())
        outs = []
        for flags in (0, _capi.WT_PLAN_FLAG_FP32_GEMM):
            (wav, _bb), _p = m._call(_capi.lib.wt_decode, _capi.WT_PLAN_DECODE, 1, 20, flags, dev, [feats], [((1, m._wave_len(20)), torch.float32, True), None],
                                 scalars=(0,))
            torch.cuda.synchronize()
            outs.append(wav.cpu().numpy())
        assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])
    m._engine.close()


# ------------------------------------------------------------------------------------------------ plans on scaled copies
K = 9
P2 = np.float32(2.0 ** K)


def _mul(sd, key, f, idx=None):
    v = sd[key].copy()
    if idx is None:
        v *= np.float32(f)
    else:
        v[idx] *= np.float32(f)
    sd[key] = v


def _set(sd, key, idx, val):
    v = sd[key].copy()
    v[idx] = val
    sd[key] = v


def _edit(sd, label):
    """One edit of a state dict, in place; returns (factor of the features, [names of the copies it moves out of the window],
    keys to plant after the conditioning check).  Exact arithmetic gives the unedited function (powers of two moved from one
    factor of a product to the other), or, for the planted ones, the function of the model with the dead channel."""
    p = "backbone.pos_net.2."
    if label == "embed":                 # W 2^-k . (x 2^k)
        _mul(sd, "backbone.embed.weight", 1 / P2)
        return float(P2), ["bb.embed.s32"], []
    if label == "pwconv2":               # gamma 2^k (W 2^-k h + b 2^-k)
        for i in (0, 3):
            _mul(sd, "backbone.convnext.%d.pwconv2.weight" % i, 1 / P2), _mul(sd, "backbone.convnext.%d.pwconv2.bias" % i, 1 / P2)
            _mul(sd, "backbone.convnext.%d.gamma" % i, P2)
        return 1.0, ["bb.cnx.0.W2.s32", "bb.cnx.3.W2.s32"], []
    if label == "pwconv1":               # W 2^-k (norm(x) s 2^k + h 2^k) + b
        _mul(sd, "backbone.convnext.1.pwconv1.weight", 1 / P2)
        _mul(sd, "backbone.convnext.1.norm.scale.weight", P2), _mul(sd, "backbone.convnext.1.norm.shift.weight", P2)
        return 1.0, ["bb.cnx.1.W1.s32"], []
    if label == "qk":
        # (q 2^-k) . (k 2^k): the scores are unchanged.  With the synthetic weights (|w| <= 0.242) that alone leaves q | k at a
        # maximum of 124, inside the window (and k = -14 at 3932, still inside, with q's activations beyond the f16 range), so
        # the block's norm is scaled by 2^-6 and the three weights that read it by 2^6 as well: q | k at 7923, above the window
        for t, f in (("q", 1 / P2), ("k", P2)):
            _mul(sd, p + t + ".weight", f * 64), _mul(sd, p + t + ".bias", f)
        _mul(sd, p + "v.weight", 64)
        _mul(sd, p + "norm.weight", 1 / 64), _mul(sd, p + "norm.bias", 1 / 64)
        return 1.0, ["bb.attn.Wqk.s32"], []
    if label == "v_proj":                # Wp 2^k (P (Wv 2^-k h + bv 2^-k)): plan.cpp sets at_Wv's acc_scale by hand (V^T = Wv . h^T)
        _mul(sd, p + "v.weight", 1 / P2), _mul(sd, p + "v.bias", 1 / P2), _mul(sd, p + "proj_out.weight", P2)
        return 1.0, ["bb.attn.Wv.s32"], []
    if label == "head":                  # the final LayerNorm's channel DEAD is exactly zero; the head weight reads it through 2^13
        _set(sd, "backbone.final_layer_norm.weight", DEAD, 0.0), _set(sd, "backbone.final_layer_norm.bias", DEAD, 0.0)
        return 1.0, ["head.W.s32"], [("head.out.weight", (11, DEAD))]
    if label == "conv2":                 # swish(GroupNorm 2) of every pos_net resblock: channel DEAD exactly zero
        plants = []
        for i in (0, 1, 3, 4):
            _set(sd, "backbone.pos_net.%d.norm2.weight" % i, DEAD, 0.0), _set(sd, "backbone.pos_net.%d.norm2.bias" % i, DEAD, 0.0)
            plants.append(("backbone.pos_net.%d.conv2.weight" % i, (13, DEAD, 1)))
        return 1.0, ["bb.res.%d.c2.s32" % i for i in range(4)], plants
    raise KeyError(label)


EDITS = ["embed", "pwconv2", "pwconv1", "qk", "v_proj", "head", "conv2"]
_CASES = {}


def _case(name, label):
    """(edited dict, features (2, 50), copies that must be scaled, decode_reference on them): computed once on the CPU, shared.
    The float64 oracle on the edited dict matches the one before the edit (unedited, or with the dead channels only) to 1e-12."""
    if (name, label) in _CASES:
        return _CASES[(name, label)]
    sd = dict(synth_state_dict(name))
    feats = range_ref.features(2, 50)
    scaled, plants, f = [], [], 1.0
    for lb in (EDITS if label == "all" else [label]):
        fi, si, pi = _edit(sd, lb)
        f, scaled, plants = f * fi, scaled + si, plants + pi
    feats = feats * f
    _o32, o64 = range_ref.oracles(name, sd)
    with torch.inference_mode():
        before = o64.decode(feats.double(), BW).numpy()
    if not plants:
        base = range_ref.reference(name, 2, 50)["w64"]
        assert rel_l2(before, base) < 1e-12, (label, rel_l2(before, base))
    for key, idx in plants:
        _set(sd, key, idx, np.float32(2.0 ** 13))
    ref = range_ref.decode_reference(name, sd, feats)
    assert rel_l2(ref["w64"], before) < 1e-12, (label, rel_l2(ref["w64"], before))
    _CASES[(name, label)] = (sd, feats, scaled, ref)
    return _CASES[(name, label)]


def _assert_scaled(model, names):
    got = {w.name.decode(): w.acc_scale for w in _infos(model)}
    for n in names:
        assert got[n] != 1.0, (n, "is not on the scaled route: the case proves nothing")
    return {n: got[n] for n in names}


@gpu
@pytest.mark.parametrize("label", EDITS)
@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_decode_on_scaled_copies(name, label):
    """The shipped decode plan at (2, 50) with one GEMM weight's copy on the scaled route (below the window for k = 9, above it
    for the planted 2^13 and for q | k), at test_precision_against_float64's bars.

    Measured on an MI355X, rel-L2 from float64 (multiple of the CPU fp32 oracle's on the same model), hop600 / hop320:
    embed 3.24e-6 (1.27) / 3.29e-6 (1.27), pwconv2 3.27e-6 (1.28) / 3.32e-6 (1.29), pwconv1 3.28e-6 (1.28) / 3.32e-6 (1.29),
    qk 3.34e-6 (1.31) / 3.39e-6 (1.31), v_proj 3.29e-6 (1.29) / 3.33e-6 (1.29), head 3.27e-6 (1.28) / 3.31e-6 (1.29),
    conv2 3.31e-6 (1.41) / 3.30e-6 (1.41).
    While s32_weight_scale brought a maximum above the window into [1, 2), conv2 missed the 4x bar: 1.495e-5 (6.36) / 1.559e-5
    (6.64), with qk at 1.98 and head at 1.38.  One element of 2^13 brought the whole tensor down by 2^-13, the other weights of
    pos_net's convs (|w| <= 0.071, typically 0.02) landed near 2^-18.6 and kept the split form's absolute floor of 2^-36: 17 bits
    instead of 22.  The rule now lowers such a maximum into [2^11, 2^12) only."""
    from wavtokenizer_amd import NAMED_ARCHS
    sd, feats, scaled, ref = _case(name, label)
    m = _fresh(NAMED_ARCHS[name], sd)
    acc = _assert_scaled(m._engine.model, scaled)
    out = m.decode(feats.cuda(), bandwidth_id=BW).cpu().numpy()
    e = range_ref.float64_bars(out, ref, f"scaled copies {name} {label} {acc}")
    assert np.isfinite(out).all() and e > 0
    _quiet(m)
    m._engine.close()


@gpu
@pytest.mark.parametrize("plan", ["f16x3", "f16", "codes"])
@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_decode_on_all_scaled_copies_together(name, plan):
    """All edits at once: on the f16x3 plan (float64 bars), on the F16_GEMM plan (test_decode_f16's bars: within 3x either way of
    the error f16_ref.decode_f64 gives for this model and these features with every operand rounded to its hi half) and through
    decode_codes (the embed edit's 2^9 moved into the codebook, whose rows are the features; float64 bars).

    Measured on an MI355X, hop600 / hop320: f16x3 3.22e-6 (1.37 x the CPU fp32 oracle) / 3.24e-6 (1.39 x); decode_codes 3.45e-6
    (1.53 x) / 3.54e-6 (1.60 x); F16_GEMM 3.10e-3 = 1.04 E / 3.12e-3 = 1.07 E.  (With maxima above the window brought into [1, 2):
    6.83 x / 7.13 x, 7.28 x / 7.23 x, and E ten times as large: test_decode_on_scaled_copies' docstring.)"""
    from wavtokenizer_amd import NAMED_ARCHS
    arch = NAMED_ARCHS[name]
    sd, feats, scaled, ref = _case(name, "all")
    if plan == "codes":
        sd = dict(sd)
        _mul(sd, (W.VQ % 0) + "embed", P2)
        codes = torch.from_numpy(np.random.default_rng(4).integers(0, arch.vq_bins, size=(1, 2, 50)))
        _o32, o64 = range_ref.oracles(name, sd)
        _b32, b64 = range_ref.oracles(name, synth_state_dict(name))
        with torch.inference_mode():
            fc = o64.codes_to_features(codes)
            assert torch.equal(fc, b64.codes_to_features(codes) * float(P2))
        ref = range_ref.decode_reference(name, sd, fc.float())
    m = _fresh(arch, sd)
    acc = _assert_scaled(m._engine.model, scaled)
    try:
        if plan == "codes":
            out = m.decode_codes(codes.cuda(), bandwidth_id=BW).cpu().numpy()
            range_ref.float64_bars(out, ref, f"scaled copies {name} all, decode_codes")
        elif plan == "f16x3":
            out = m.decode(feats.cuda(), bandwidth_id=BW).cpu().numpy()
            range_ref.float64_bars(out, ref, f"scaled copies {name} all {acc}")
        else:
            with torch.inference_mode():
                E = f16_ref.rel_l2(f16_ref.decode_f64(arch, sd, feats.double(), 0, q=True), ref["w64"])
            m.set_gemm_precision("f16")
            err = rel_l2(m.decode(feats.cuda(), bandwidth_id=BW).cpu().numpy(), ref["w64"])
            print(f"scaled copies {name} all, F16_GEMM plan: rel-L2 {err:.3e} from float64, emulated E {E:.3e} ({err / E:.2f} E)")
            assert E / 3 <= err <= 3 * E, (err, E)
        _quiet(m)
    finally:
        m._engine.close()


def _two_frame_T(name):
    from wavtokenizer_amd import NAMED_ARCHS
    hop = NAMED_ARCHS[name].hop
    return min(T for T in manifest()["archs"][name]["cases"]["edge"]["T"] if -(-T // hop) == 2)


def _enc_last_down(arch):
    return W.ENC + "%d.conv.conv" % (3 * len(arch.ratios))


_ENC = {}


def _encode_case(name, label):
    """(edited dict, wav, float64 codes, margins, float64 features) of an encoder edit, on the CPU, once."""
    from wavtokenizer_amd import NAMED_ARCHS, synth
    if (name, label) in _ENC:
        return _ENC[(name, label)]
    arch = NAMED_ARCHS[name]
    sd = dict(synth_state_dict(name))
    wav = torch.from_numpy(synth.make_clips(2, _two_frame_T(name), seed=31))
    final = W.ENC + "%d.conv.conv" % (3 * len(arch.ratios) + 3)          # (behind the LSTM at 3 n + 1 and its ELU)
    assert final + ".weight_g" in sd and sd[final + ".weight_v"].shape[2] == 7

    def run(d):
        _o32, o64 = range_ref.oracles(name, d)
        taps = {}
        with torch.inference_mode():
            f, c = o64.encode_infer(wav.double(), BW, taps)
        return f.numpy(), c.numpy(), taps["vq.margin"].numpy()

    if label == "final+codebook":        # emb 2^-k against a codebook 2^-k: the same nearest rows, the features times 2^-k
        f0, c0, m0 = run(sd)
        _mul(sd, final + ".weight_g", 1 / P2), _mul(sd, final + ".bias", 1 / P2), _mul(sd, (W.VQ % 0) + "embed", 1 / P2)
        f1, c1, _m1 = run(sd)
        assert np.array_equal(c1, c0) and rel_l2(f1 * float(P2), f0) < 1e-12
        out = (sd, wav, c0, m0, f1, ["enc.final.s32", "vq.embed.s32"])
    else:                                # Wih0: the LSTM's input channel DEAD is exactly zero (the last down conv's g and bias)
        down = _enc_last_down(arch)
        _set(sd, down + ".weight_g", (DEAD, 0, 0), 0.0), _set(sd, down + ".bias", DEAD, 0.0)
        f0, c0, m0 = run(sd)
        _set(sd, W.ENC + "%d.lstm.weight_ih_l0" % (3 * len(arch.ratios) + 1), (17, DEAD), np.float32(2.0 ** 13))
        f1, c1, _m1 = run(sd)
        assert np.array_equal(c1, c0) and rel_l2(f1, f0) < 1e-12
        out = (sd, wav, c0, m0, f1, ["enc.lstm.Wih0.s32"])
    _ENC[(name, label)] = out
    return out


@gpu
@pytest.mark.parametrize("label", ["final+codebook", "Wih0"])
@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_encode_on_scaled_copies(name, label):
    """Two frames per clip.  The codes equal the float64 oracle's by check_codes' near-tie rule, with the margins of the model
    before the scaling (the scaled model's distances, and so its margins, are 2^-18 times those), and the features are the
    scaled codebook's rows exactly."""
    from wavtokenizer_amd import NAMED_ARCHS
    sd, wav, codes64, margin, feats64, scaled = _encode_case(name, label)
    m = _fresh(NAMED_ARCHS[name], sd)
    acc = _assert_scaled(m._engine.model, scaled)
    feats, codes = m.encode_infer(wav.cuda(), bandwidth_id=BW)
    flips = check_codes(codes.cpu().numpy(), codes64, margin, f"{name} {label}")
    book = torch.from_numpy(sd[(W.VQ % 0) + "embed"])
    assert torch.equal(feats.cpu(), book[codes.cpu()[0]].transpose(1, 2)), "features are not the (scaled) codebook's rows"
    if flips == 0:
        assert np.array_equal(feats.cpu().numpy().astype(np.float64), feats64)
    print(f"encode on scaled copies {name} {label}: {acc}, {flips} near-tie flips of {codes64.size}")
    _quiet(m)
    m._engine.close()
