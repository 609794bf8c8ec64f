"""Decode straight from codes (WT_PLAN_DECODE_CODES / _MIXED, wt_decode_codes / wt_decode_codes_mixed, WavTokenizer.decode_codes /
decode_codes_many) on the GPU: every waveform is the bits of today's composition decode(codes_to_features(codes)), on every
route a decode plan takes, and within the project's waveform bar of the reference's own composition."""
import ctypes
import dataclasses
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _load(arch, sd):
    from wavtokenizer_amd import WavTokenizer
    m = WavTokenizer.from_arch(arch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m.eval().to("cuda")


_MODELS = {}


def _cached(name):
    """hop600 / hop320 with synthetic weights (as tests/test_decode_many.py); "hop600q3": hop600 with three codebooks."""
    from wavtokenizer_amd import NAMED_ARCHS, synth
    if name not in _MODELS:
        arch = dataclasses.replace(NAMED_ARCHS["hop600"], num_quantizers=3) if name == "hop600q3" else NAMED_ARCHS[name]
        _MODELS[name] = _load(arch, synth.make_state_dict(arch, seed=321))
    return _MODELS[name]


@pytest.fixture(scope="module", params=["hop600", "hop320"])
def model(request):
    return request.param, _cached(request.param)


def _codes(m, K, B, L, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, m.arch.vq_bins, size=(K, B, L))).cuda()


def _bw(i):
    return torch.tensor([i])


def _compose(m, codes, bw):
    return m.decode(m.codes_to_features(codes), bandwidth_id=_bw(bw))


def _no_status(m):
    m.check_status()
    assert not m.fallback_events


def _plans(m, kind):
    return [(k, p) for k, (p, _ws) in m._engine.plans.items() if k[0] == kind]


# ------------------------------------------------------------------------------------------- bits of the composition
SHAPES = [(1, 1), (1, 2), (2, 33), (3, 129), (17, 40)]       # (17, 40) is above the graph limit of 16 clips


@pytest.mark.parametrize("bw", [0, 2])
def test_decode_codes_is_the_bits_of_the_composition(model, bw):
    from wavtokenizer_amd import _capi
    name, m = model
    for B, L in SHAPES:
        codes = _codes(m, 1, B, L, seed=B * 1000 + L)
        want = _compose(m, codes, bw)
        assert want.shape == (B, m._wave_len(L)) and bool(torch.isfinite(want).all())
        for _rep in range(3 if B <= 16 else 1):              # the second call records the graph, it and the third replay it
            got = m.decode_codes(codes, bandwidth_id=_bw(bw))
            assert got.shape == want.shape and torch.equal(got, want), (name, B, L, _rep)
        if B == 1:                                           # the (K, L) layout of codes_to_features
            assert torch.equal(m.decode_codes(codes[:, 0, :], bandwidth_id=_bw(bw)), want), (name, L)
        (key, plan), = [(k, p) for k, p in _plans(m, _capi.WT_PLAN_DECODE_CODES) if k[1] == B and k[2] == L]
        assert bool(key[3] & _capi.WT_PLAN_FLAG_GRAPH) == (B <= 16)
        if B <= 16:
            assert _capi.lib.wt_plan_graph_replays(plan) >= 2, (name, B, L)
    _no_status(m)


def test_k_is_an_argument_of_the_call_and_of_the_graph_key():
    from wavtokenizer_amd import _capi
    m = _cached("hop600q3")
    B, L = 2, 33
    for K in (1, 2, 3):
        codes = _codes(m, K, 3, 20, seed=K)
        assert torch.equal(m.decode_codes(codes, bandwidth_id=_bw(0)), _compose(m, codes, 0)), K
    c2 = _codes(m, 2, 1, 19, seed=9)[:, 0, :]
    assert torch.equal(m.decode_codes(c2, bandwidth_id=_bw(1)), _compose(m, c2, 1))
    # one plan, one staging buffer, one recording at a time: a replay recorded for K = 1 must never serve a K = 3 call
    c1, c3 = _codes(m, 1, B, L, seed=21), _codes(m, 3, B, L, seed=23)
    w1, w3 = _compose(m, c1, 0), _compose(m, c3, 0)
    assert not torch.equal(w1, w3)
    for K in (1, 1, 1, 3, 3, 3, 1, 3, 1, 1, 1):
        got = m.decode_codes(c1 if K == 1 else c3, bandwidth_id=_bw(0))
        assert torch.equal(got, w1 if K == 1 else w3), K
    (key, plan), = [(k, p) for k, p in _plans(m, _capi.WT_PLAN_DECODE_CODES) if k[1] == B and k[2] == L]
    assert _capi.lib.wt_plan_graph_replays(plan) >= 4
    with pytest.raises(_capi.WavTokError, match="K must be"):
        m.decode_codes(torch.zeros(4, 1, 7, dtype=torch.int64, device="cuda"), bandwidth_id=_bw(0))     # more code rows than codebooks
    _no_status(m)


def test_off_the_shipped_route(model):
    """fp32 GEMMs, and the unfused debug plans with their stage taps: the same bit equality, one small shape each."""
    name, m = model
    codes = _codes(m, 1, 2, 33, seed=77)
    try:
        m.set_gemm_precision("f32")
        assert torch.equal(m.decode_codes(codes, bandwidth_id=_bw(0)), _compose(m, codes, 0))
        m.set_gemm_precision("f16x3")
        m.set_debug_keep_stages(True, unfused=True)
        assert torch.equal(m.decode_codes(codes[:, :1, :5], bandwidth_id=_bw(2)), _compose(m, codes[:, :1, :5], 2))
        m.set_debug_keep_stages(True)
        assert torch.equal(m.decode_codes(codes[:, :1, :5], bandwidth_id=_bw(2)), _compose(m, codes[:, :1, :5], 2))
    finally:
        m.set_gemm_precision("f16x3")
        m.set_debug_keep_stages(False)
    _no_status(m)


# --------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_against_the_reference_composition(name):
    from oracle.cpu_ref import OracleWavTokenizer
    from tests.util import WAV_REL_TOL, load_case, rel_l2, synth_state_dict
    from wavtokenizer_amd import NAMED_ARCHS
    assert WAV_REL_TOL == 1e-4
    arch, sd = NAMED_ARCHS[name], synth_state_dict(name)
    m = _load(arch, sd)
    orc = OracleWavTokenizer(arch, sd)
    ragged = int(load_case(name, "b1_t61920")["codes"].shape[-1])          # frames of the 61920-sample clip
    assert ragged == arch.frames(61920)
    gen = torch.Generator().manual_seed(5)
    for B, L in ((2, 120), (1, ragged)):
        codes = torch.randint(0, arch.vq_bins, (1, B, L), generator=gen)
        with torch.inference_mode():
            ref = orc.decode(orc.codes_to_features(codes), _bw(0))
        got = m.decode_codes(codes.cuda(), bandwidth_id=_bw(0))
        err = rel_l2(got.cpu().numpy(), ref.numpy())
        print(f"decode_codes oracle {name} B={B} L={L}: rel_l2 {err:.3e}")
        assert got.shape == ref.shape and err <= WAV_REL_TOL, (name, B, L, err)
    if name == "hop600":
        g = load_case(name, "b2_t72000")                   # codes and waveform captured from the reference
        got = m.decode_codes(torch.from_numpy(g["codes"]).cuda(), bandwidth_id=_bw(0))
        err = rel_l2(got.cpu().numpy(), g["wav_out"])
        print(f"decode_codes golden {name}: rel_l2 {err:.3e}")
        assert err <= WAV_REL_TOL, err


# ------------------------------------------------------------------------------------------------ decode_codes_many
SET_A = [1, 2, 3, 7, 31, 32, 33, 127, 128, 129, 255, 256]
SET_B = [200, 256, 257, 300, 384, 385, 400]


def _clips(m, frames, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, m.arch.vq_bins, size=(1, int(L)))).cuda() for L in frames]


_SOLO = {}


def _solo(m, clips, bw, key):
    """decode_codes of every clip alone: computed once per (model, set, bandwidth), shared, never modified."""
    k = (id(m), key, bw)
    if k not in _SOLO:
        _SOLO[k] = [m.decode_codes(c, bandwidth_id=_bw(bw)) for c in clips]
    return _SOLO[k]


@pytest.mark.parametrize("frames,key", [(SET_A, "a"), (SET_B, "b")])
def test_decode_codes_many(model, frames, key):
    from wavtokenizer_amd import _capi
    name, m = model
    clips = _clips(m, frames, seed=len(frames))
    solo = _solo(m, clips, 1, key)
    order = list(range(len(frames)))
    random.Random(3).shuffle(order)
    got = m.decode_codes_many([clips[i] if j % 2 else clips[i][:, None, :] for j, i in enumerate(order)], bandwidth_id=_bw(1))
    feats = [m.codes_to_features(clips[i])[0] for i in order]
    many = m.decode_many(feats, bandwidth_id=_bw(1))
    for j, i in enumerate(order):
        assert got[j].shape == (1, m._wave_len(frames[i]))
        assert torch.equal(got[j], solo[i]), (name, frames[i])
        assert torch.equal(got[j], many[j]), (name, frames[i])
    assert _plans(m, _capi.WT_PLAN_DECODE_CODES_MIXED)
    _no_status(m)


def _assert_clips(m, wav, clips, ref):
    assert wav.shape[0] == len(clips)
    for j, (c, r) in enumerate(zip(clips, ref)):
        n = m._wave_len(int(c.shape[1]))
        assert torch.equal(wav[j:j + 1, :n], r), (j, int(c.shape[1]))
        assert bool((wav[j, n:] == 0).all()), (j, int(c.shape[1]))


@pytest.mark.parametrize("frames,key,L_pad", [(SET_A, "a", 256), (SET_B, "b", 400)])
def test_staging_past_a_clip_does_not_matter(model, frames, key, L_pad):
    from wavtokenizer_amd import _capi
    name, m = model
    clips = _clips(m, frames, seed=len(frames))
    solo = _solo(m, clips, 1, key)
    B = len(clips)
    wav = m._run_decode_codes_mixed(clips, L_pad, 1)
    assert wav is not None and wav.shape == (B, m._wave_len(L_pad))
    _assert_clips(m, wav, clips, solo)
    # the plan's staging buffer (a graph plan keeps one): -1 and 2^62 everywhere; the next call writes each clip's own codes only
    (kp, plan), = [(k, p) for k, p in _plans(m, _capi.WT_PLAN_DECODE_CODES_MIXED) if k[1] == B and k[2] == L_pad]
    assert kp[3] & _capi.WT_PLAN_FLAG_GRAPH
    staging = m._engine.io[plan.value][0][0]
    assert staging.dtype == torch.int64 and staging.shape[1:] == (B, L_pad)
    for _round in range(2):                                  # (the second of them replays the recording)
        with torch.inference_mode():                         # (the staging buffers are made under it)
            staging.view(-1)[0::2] = -1
            staging.view(-1)[1::2] = 2 ** 62
        wav = m._run_decode_codes_mixed(clips, L_pad, 1)     # (set_check_codes is "sync": a flagged index would raise here)
        _assert_clips(m, wav, clips, solo)
        for j, c in enumerate(clips):
            assert bool((staging[0, j, c.shape[1]:] != 0).all())      # the pad codes are still what the test left there
    _no_status(m)


def test_off_route_goes_clip_by_clip():
    from wavtokenizer_amd import _capi
    m = _cached("hop320")
    clips = _clips(m, [3, 50, 41, 300], seed=4)
    try:
        m.set_gemm_precision("f32")
        assert m._run_decode_codes_mixed(clips[:2], 64, 0) is None
        got = m.decode_codes_many(clips, bandwidth_id=_bw(0))
        for g, c in zip(got, clips):
            assert torch.equal(g, _compose(m, c, 0))
        assert not [k for k, _p in _plans(m, _capi.WT_PLAN_DECODE_CODES_MIXED) if k[3] & _capi.WT_PLAN_FLAG_FP32_GEMM]
    finally:
        m.set_gemm_precision("f16x3")
    _no_status(m)


# --------------------------------------------------------------------------------------------------- bad indices
def test_bad_index_inside_a_clip():
    from wavtokenizer_amd import _capi
    m = _cached("hop600")
    clips = _clips(m, [20, 33, 40], seed=8)
    solo = [m.decode_codes(c, bandwidth_id=_bw(0)) for c in clips]
    bad = [c.clone() for c in clips]
    bad[1][0, 7] = m.arch.vq_bins
    try:
        # "sync" (the default): the offending call raises, as F.embedding does
        assert m._check_codes == "sync"
        with pytest.raises(IndexError, match="index out of range in self"):
            m.decode_codes(bad[1], bandwidth_id=_bw(0))
        with pytest.raises(IndexError, match="index out of range in self"):
            m.decode_codes_many(bad, bandwidth_id=_bw(0))
        assert torch.equal(m.decode_codes(clips[1], bandwidth_id=_bw(0)), solo[1])      # (the flag was consumed)
        # "off", one mixed call: that clip is NaN, the others and the call's status are not affected
        m.set_check_codes("off")
        wav = m._run_decode_codes_mixed(bad, 40, 0)
        torch.cuda.synchronize()
        for j, c in enumerate(clips):
            n = m._wave_len(int(c.shape[1]))
            if j == 1:
                assert bool(torch.isnan(wav[j, :n]).all())
            else:
                assert torch.equal(wav[j:j + 1, :n], solo[j]), j
            assert bool((wav[j, n:] == 0).all()), j
        _no_status(m)
        assert _capi.lib.wt_model_take_bad_codes(m._engine.model) == 1      # (left there in this mode: taken before going on)
        # "deferred": the call returns, the error arrives on the next call
        m.set_check_codes("deferred")
        w = m.decode_codes(bad[1], bandwidth_id=_bw(0))
        torch.cuda.synchronize()
        assert bool(torch.isnan(w).all())
        with pytest.raises(IndexError, match="index out of range in self"):
            m.decode_codes(clips[0], bandwidth_id=_bw(0))
        assert torch.equal(m.decode_codes(clips[0], bandwidth_id=_bw(0)), solo[0])
    finally:
        m.set_check_codes("sync")
        _capi.lib.wt_model_take_bad_codes(m._engine.model)
    _no_status(m)


# ---------------------------------------------------------------------------------------------- the plan and the ABI
def _step_names(lib, plan):
    out = []
    for i in range(lib.wt_plan_num_steps(plan)):
        s = ctypes.c_char_p()
        assert lib.wt_plan_step_name(plan, i, ctypes.byref(s)) == 0
        out.append(s.value.decode())
    return out


def _buffer(lib, plan, name):
    off, n, fmt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
    assert lib.wt_plan_buffer_info(plan, name.encode(), ctypes.byref(off), ctypes.byref(n), ctypes.byref(fmt)) == 0
    off2, n2 = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.wt_plan_find_buffer(plan, name.encode(), ctypes.byref(off2), ctypes.byref(n2)) == 0 and n2.value == n.value
    return n.value, fmt.value


@pytest.mark.parametrize("flags", [0, 2])                   # the shipped route, and WT_PLAN_FLAG_FP32_GEMM (bb.in in fp32)
def test_plan_is_the_decode_plan_with_its_first_step_replaced(model, flags):
    from wavtokenizer_amd import _capi
    name, m = model
    m._ensure_engine()
    lib = _capi.lib
    dev = torch.device("cuda", torch.cuda.current_device())
    B, L = 2, 33
    pd, _ws = m._engine.plan(_capi.WT_PLAN_DECODE, B, L, flags, dev)
    pc, _ws = m._engine.plan(_capi.WT_PLAN_DECODE_CODES, B, L, flags, dev)
    assert lib.wt_plan_num_launches(pc) == lib.wt_plan_num_launches(pd)
    sd, sc = _step_names(lib, pd), _step_names(lib, pc)
    assert len(sd) == len(sc)
    assert "code_rows" in sc and "code_rows" not in sd
    assert "bb.in" in sd and "bb.in" not in sc               # (the transpose step carries its buffer's name)
    assert [s for s in sc if s != "code_rows"] == [s for s in sd if s != "bb.in"]
    assert _buffer(lib, pc, "bb.in") == _buffer(lib, pd, "bb.in") == (B * L * 512, 0 if flags else _capi.BUF_S32)
    pm, _ws = m._engine.plan(_capi.WT_PLAN_DECODE_CODES_MIXED, B, L, 0, dev)
    sm = _step_names(lib, pm)
    assert "mix.lengths" in sm and "code_rows" in sm and "bb.in" not in sm


@pytest.mark.parametrize("what", ["range_report", "fp32_site", "fp32_site_attn", "fp32_site_cnx1", "fp32_site_head", "step_lstm_flag"])
def test_every_decode_plan_variant_runs_from_codes(what):
    """WT_PLAN_FLAG_RANGE_REPORT (code_rows feeds the report with bb.in), backbone.embed on fp32 operands (bb.in in fp32 on an
    otherwise split-f16 plan), a range site behind it on fp32 operands (bb.in stays split-f16), and a flag the decoder ignores:
    the codes plan and the features plan of the same flags and sites return the same bits."""
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.pretrained import _ptr, _stream_ptr
    m = _cached("hop600")
    m._ensure_engine()
    lib = _capi.lib
    dev = torch.device("cuda", torch.cuda.current_device())
    B, L = 2, 33
    flags, sites = {"range_report": (_capi.WT_PLAN_FLAG_RANGE_REPORT, 0), "fp32_site": (0, 1 << _capi.WT_SITE_BB_EMBED),
                    "fp32_site_attn": (0, 1 << _capi.WT_SITE_ATTN), "fp32_site_cnx1": (0, 1 << (_capi.WT_SITE_CNX0 + 1)),
                    "fp32_site_head": (0, 1 << _capi.WT_SITE_HEAD), "step_lstm_flag": (_capi.WT_PLAN_FLAG_STEP_LSTM, 0)}[what]
    codes = _codes(m, 1, B, L, seed=3)
    feats = m.codes_to_features(codes)
    pd, wsd = m._engine.plan(_capi.WT_PLAN_DECODE, B, L, flags, dev, sites)
    pc, wsc = m._engine.plan(_capi.WT_PLAN_DECODE_CODES, B, L, flags, dev, sites)
    wd = torch.empty((B, m._wave_len(L)), device=dev)
    wc = torch.empty_like(wd)
    bbd = torch.empty((B, L, m.arch.dim), device=dev)
    bbc = torch.empty_like(bbd)
    st = _stream_ptr(dev)
    _capi.check(lib.wt_decode(pd, _ptr(feats), 2, _ptr(wd), _ptr(bbd), _ptr(wsd), st), "wt_decode")
    _capi.check(lib.wt_decode_codes(pc, _ptr(codes), 1, 2, _ptr(wc), _ptr(bbc), _ptr(wsc), st), "wt_decode_codes")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(wd).all()) and torch.equal(wc, wd) and torch.equal(bbc, bbd)      # (the backbone output too)
    assert _buffer(lib, pc, "bb.in")[1] == (0 if sites & (1 << _capi.WT_SITE_BB_EMBED) else _capi.BUF_S32)
    if sites:                                                # (the site is in force: other bits than the shipped plan's)
        p0, ws0 = m._engine.plan(_capi.WT_PLAN_DECODE_CODES, B, L, 0, dev)
        w0 = torch.empty_like(wd)
        _capi.check(lib.wt_decode_codes(p0, _ptr(codes), 1, 2, _ptr(w0), _ptr(None), _ptr(ws0), st), "wt_decode_codes")
        torch.cuda.synchronize()
        assert not torch.equal(w0, wc)
    if what == "range_report":
        step, buf, amax = ctypes.c_char_p(), ctypes.c_char_p(), ctypes.c_float()
        assert lib.wt_plan_range_report(pc, 0, ctypes.byref(step), ctypes.byref(buf), ctypes.byref(amax)) == 0
        assert (step.value, buf.value) == (b"code_rows", b"bb.in")
        want = float(feats.abs().max())                      # the largest feature, to the 22 bits of the S32 form
        assert abs(amax.value - want) <= want * 2.0 ** -21, (amax.value, want)
        m._engine.drop(lambda k: k[3] & _capi.WT_PLAN_FLAG_RANGE_REPORT)
    _no_status(m)


def test_abi_refusals_touch_nothing():
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.pretrained import _ptr, _stream_ptr
    m = _cached("hop600q3")
    m._ensure_engine()
    lib = _capi.lib
    dev = torch.device("cuda", torch.cuda.current_device())
    B, L = 2, 40
    plain, wsp = m._engine.plan(_capi.WT_PLAN_DECODE, B, L, 0, dev)
    cod, wsc = m._engine.plan(_capi.WT_PLAN_DECODE_CODES, B, L, 0, dev)
    mix, wsm = m._engine.plan(_capi.WT_PLAN_DECODE_CODES_MIXED, B, L, 0, dev)
    codes = _codes(m, 3, B, L, seed=1)
    x = torch.zeros((B, 512, L), device=dev)
    lens = torch.tensor([L, 7], dtype=torch.int32, device=dev)
    wav = torch.full((B, m._wave_len(L)), 7.0, device=dev)
    st = _stream_ptr(dev)
    null = _ptr(None)
    calls = [
        ("a features plan", lambda: lib.wt_decode_codes(plain, _ptr(codes), 1, 0, _ptr(wav), null, _ptr(wsp), st), b"WT_PLAN_DECODE_CODES"),
        ("a mixed plan", lambda: lib.wt_decode_codes(mix, _ptr(codes), 1, 0, _ptr(wav), null, _ptr(wsm), st), b"wt_decode_codes_mixed"),
        ("wt_decode on a codes plan", lambda: lib.wt_decode(cod, _ptr(x), 0, _ptr(wav), null, _ptr(wsc), st), b"not a decode plan"),
        ("mixed entry, plain plan", lambda: lib.wt_decode_codes_mixed(cod, _ptr(codes), 1, _ptr(lens), 0, _ptr(wav), _ptr(wsc), st), b"mixed-length"),
        ("mixed entry, features plan", lambda: lib.wt_decode_mixed(mix, _ptr(x), _ptr(lens), 0, _ptr(wav), _ptr(wsm), st), b"mixed-length"),
        ("K = 0", lambda: lib.wt_decode_codes(cod, _ptr(codes), 0, 0, _ptr(wav), null, _ptr(wsc), st), b"K must be"),
        ("K = num_quantizers + 1", lambda: lib.wt_decode_codes(cod, _ptr(codes), 4, 0, _ptr(wav), null, _ptr(wsc), st), b"K must be"),
        ("null codes", lambda: lib.wt_decode_codes(cod, null, 1, 0, _ptr(wav), null, _ptr(wsc), st), b"null buffer"),
        ("mixed: K = 0", lambda: lib.wt_decode_codes_mixed(mix, _ptr(codes), 0, _ptr(lens), 0, _ptr(wav), _ptr(wsm), st), b"K must be"),
        ("mixed: K = 4", lambda: lib.wt_decode_codes_mixed(mix, _ptr(codes), 4, _ptr(lens), 0, _ptr(wav), _ptr(wsm), st), b"K must be"),
        ("mixed: null codes", lambda: lib.wt_decode_codes_mixed(mix, null, 1, _ptr(lens), 0, _ptr(wav), _ptr(wsm), st), b"null buffer"),
        ("mixed: null lengths", lambda: lib.wt_decode_codes_mixed(mix, _ptr(codes), 1, null, 0, _ptr(wav), _ptr(wsm), st), b"null buffer"),
        ("bandwidth", lambda: lib.wt_decode_codes(cod, _ptr(codes), 1, 99, _ptr(wav), null, _ptr(wsc), st), b"bandwidth_id"),
    ]
    for what, call, msg in calls:
        assert call() == _capi.WT_ERR_INVALID, what
        assert msg in lib.wt_last_error(), (what, lib.wt_last_error())
    torch.cuda.synchronize()
    assert bool((wav == 7.0).all())
    # the mixed kind carries the route restriction of WT_PLAN_DECODE_MIXED
    for flag in (_capi.WT_PLAN_FLAG_UNFUSED, _capi.WT_PLAN_FLAG_FP32_GEMM, _capi.WT_PLAN_FLAG_KEEP_STAGES, _capi.WT_PLAN_FLAG_RANGE_REPORT):
        p = ctypes.c_void_p()
        assert lib.wt_plan_create(m._engine.model, _capi.WT_PLAN_DECODE_CODES_MIXED, 2, 40, flag, ctypes.byref(p)) == _capi.WT_ERR_INVALID, flag
        assert b"mixed-length" in lib.wt_last_error()
    p = ctypes.c_void_p()
    assert lib.wt_plan_create_ex(m._engine.model, _capi.WT_PLAN_DECODE_CODES_MIXED, 2, 40, 0, 1 << _capi.WT_SITE_ATTN,
                                 ctypes.byref(p)) == _capi.WT_ERR_INVALID
    # ... and the plain kind takes them all, the range report included
    p = ctypes.c_void_p()
    flags = _capi.WT_PLAN_FLAG_RANGE_REPORT
    assert lib.wt_plan_create_ex(m._engine.model, _capi.WT_PLAN_DECODE_CODES, 2, 40, flags, 1 << _capi.WT_SITE_BB_EMBED, ctypes.byref(p)) == 0
    lib.wt_plan_destroy(p)
    _no_status(m)
