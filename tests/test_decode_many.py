"""Mixed-length decode (WT_PLAN_DECODE_MIXED, wt_decode_mixed, WavTokenizer.decode_many) on the GPU: every clip's waveform is
the bits a decode call of its own length returns, whatever the batch, order, grouping, padded length or staging contents."""
import ctypes
import dataclasses
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(name, padding=None):
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth
    arch = NAMED_ARCHS[name]
    if padding:
        arch = dataclasses.replace(arch, padding=padding)
    sd = synth.make_state_dict(arch, seed=321)
    m = WavTokenizer.from_arch(arch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m.eval().to("cuda"), sd


_MODELS = {}


def _cached(name):
    if name not in _MODELS:
        _MODELS[name] = _model(name)[0]
    return _MODELS[name]


@pytest.fixture(scope="module", params=["hop600", "hop320"])
def model(request):
    return request.param, _cached(request.param)


@pytest.fixture(scope="module")
def model600():
    return _cached("hop600")


def _feats(m, frames, seed):
    """Features (512, L) of random codes, one clip per entry of `frames`."""
    rng = np.random.default_rng(seed)
    out = []
    for L in frames:
        codes = torch.from_numpy(rng.integers(0, m.arch.vq_bins, size=(1, 1, int(L)))).cuda()
        out.append(m.codes_to_features(codes)[0].contiguous())
    return out


_SOLO = {}


def _solo(m, feats, bw, key):
    """The one-clip decode of every clip: computed once per (model, set, bandwidth) and shared, never modified."""
    k = (id(m), key, bw)
    if k not in _SOLO:
        _SOLO[k] = [m.decode(f[None], bandwidth_id=torch.tensor([bw])) for f in feats]
    return _SOLO[k]


def _assert_clips(m, wav, feats, ref):
    """wav (B, wave_len(L_pad)) of one mixed call: every clip equals its solo decode, zeros behind it."""
    assert wav.shape[0] == len(feats)
    for j, (f, r) in enumerate(zip(feats, ref)):
        n = m._wave_len(int(f.shape[1]))
        assert r.shape == (1, n)
        assert torch.equal(wav[j:j + 1, :n], r), (j, int(f.shape[1]))
        assert (wav[j, n:] == 0).all(), (j, int(f.shape[1]))


def _no_status(m):
    m.check_status()
    assert not m.fallback_events


SET_A = [1, 2, 3, 7, 31, 32, 33, 127, 128, 129, 255, 256]
SET_B = [200, 256, 257, 300, 384, 385, 400]
SET_C = [1, 640, 1200, 1281, 1300]


@pytest.mark.parametrize("bw", [0, 2])
def test_set_a_slab_groupnorm_and_softmax_reg1(model, bw):
    name, m = model
    feats = _feats(m, SET_A, seed=11)
    wav = m._run_decode_mixed(feats, 256, bw)
    assert wav is not None
    _assert_clips(m, wav, feats, _solo(m, feats, bw, "a"))
    _no_status(m)


@pytest.mark.parametrize("bw", [0, 2])
def test_set_b_both_groupnorm_forms_in_one_launch(model, bw):
    name, m = model
    feats = _feats(m, SET_B, seed=12)
    wav = m._run_decode_mixed(feats, 400, bw)
    assert wav is not None
    _assert_clips(m, wav, feats, _solo(m, feats, bw, "b"))
    _no_status(m)


@pytest.mark.parametrize("L_pad", [1300, 1312])
def test_set_c_long_clips(model600, L_pad):
    m = model600
    feats = _feats(m, SET_C, seed=13)
    for bw in (0, 2):
        wav = m._run_decode_mixed(feats, L_pad, bw)
        assert wav is not None
        _assert_clips(m, wav, feats, _solo(m, feats, bw, "c"))
    _no_status(m)


def test_set_c_softmax_reg5_at_1216(model600):
    m = model600
    feats = _feats(m, SET_C, seed=13)[:3]                # [1, 640, 1200] at L_pad = 1216: softmax_reg<5>
    for bw in (0, 2):
        wav = m._run_decode_mixed(feats, 1216, bw)
        _assert_clips(m, wav, feats, _solo(m, feats, bw, "c")[:3])
    _no_status(m)


def _mixed_call(m, feats, L_pad, bw, fill=0.0, lengths=None):
    """wt_decode_mixed on a staging tensor of our own, filled with `fill` past every clip's frames."""
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.pretrained import _ptr, _stream_ptr
    m._ensure_engine()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = len(feats)
    plan, ws = m._engine.plan(_capi.WT_PLAN_DECODE_MIXED, B, L_pad, 0, dev)
    x = torch.full((B, 512, L_pad), fill, device=dev)
    for j, f in enumerate(feats):
        x[j, :, :f.shape[1]] = f
    lens = torch.tensor(lengths if lengths is not None else [int(f.shape[1]) for f in feats], dtype=torch.int32, device=dev)
    wav = torch.full((B, m._wave_len(L_pad)), 7.0, device=dev)
    _capi.check(_capi.lib.wt_decode_mixed(plan, _ptr(x), _ptr(lens), bw, _ptr(wav), _ptr(ws), _stream_ptr(dev)), "wt_decode_mixed")
    torch.cuda.synchronize()
    return wav, plan


def test_staging_contents_and_padded_length_do_not_matter(model):
    name, m = model
    feats = _feats(m, SET_B, seed=12)
    ref = _solo(m, feats, 0, "b")
    for L_pad, fill in ((400, float("nan")), (448, 0.0), (448, 1e30)):
        wav, _plan = _mixed_call(m, feats, L_pad, 0, fill)
        _assert_clips(m, wav, feats, ref)
    _no_status(m)


def test_decode_many_public(model):
    name, m = model
    rng = random.Random(7)
    frames = [rng.randint(1, 700) for _ in range(20)]
    rng.shuffle(frames)
    feats = _feats(m, frames, seed=40)
    bw = torch.tensor([1])
    ref = [m.decode(f[None], bandwidth_id=bw) for f in feats]
    got = m.decode_many([f if i % 2 else f[None] for i, f in enumerate(feats)], bandwidth_id=bw)
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape == (1, m._wave_len(frames[i])) and torch.equal(g, r), (i, frames[i])
    from wavtokenizer_amd import _capi
    assert any(k[0] == _capi.WT_PLAN_DECODE_MIXED for k in m._engine.plans)
    _no_status(m)


def test_encode_infer_many_then_decode_many_equals_the_file_loop(model):
    from wavtokenizer_amd import synth
    name, m = model
    lengths = [1024, 5000, 7777, 20000, 2500]
    wavs = [torch.from_numpy(np.ascontiguousarray(synth.make_clips(1, T, seed=70 + i)[0])).cuda() for i, T in enumerate(lengths)]
    bw = torch.tensor([0])
    many = m.decode_many([f for f, _c in m.encode_infer_many(wavs, bandwidth_id=bw)], bandwidth_id=bw)
    for w, g in zip(wavs, many):
        f, _c = m.encode_infer(w[None], bandwidth_id=bw)
        assert torch.equal(g, m.decode(f, bandwidth_id=bw))
    _no_status(m)


def test_center_padding():
    m, _sd = _model("hop600", padding="center")
    frames = [2, 5, 40, 257]
    feats = _feats(m, frames, seed=21)
    ref = [m.decode(f[None], bandwidth_id=torch.tensor([0])) for f in feats]
    wav = m._run_decode_mixed(feats, 257, 0)
    _assert_clips(m, wav, feats, ref)
    wav, _plan = _mixed_call(m, feats, 288, 0, float("nan"))
    _assert_clips(m, wav, feats, ref)
    _no_status(m)


def test_graph_replay_serves_every_length_set(model):
    from wavtokenizer_amd import _capi
    name, m = model
    sets = [[128, 5, 77, 100], [1, 128, 33, 64]]
    feats = [_feats(m, s, seed=60 + i) for i, s in enumerate(sets)]
    refs = [[m.decode(f[None], bandwidth_id=torch.tensor([0])) for f in fs] for fs in feats]
    m._engine.drop(lambda k: k[0] == _capi.WT_PLAN_DECODE_MIXED)
    for _round in range(2):
        for fs, ref in zip(feats, refs):
            _assert_clips(m, m._run_decode_mixed(fs, 128, 0), fs, ref)
    keys = [k for k in m._engine.plans if k[0] == _capi.WT_PLAN_DECODE_MIXED]
    assert len(keys) == 1 and keys[0][3] & _capi.WT_PLAN_FLAG_GRAPH, keys
    assert _capi.lib.wt_plan_graph_replays(m._engine.plans[keys[0]][0]) >= 2      # calls 2 .. 4 replay the recording
    _no_status(m)


def test_oracle():
    from oracle.cpu_ref import OracleWavTokenizer
    from tests.util import WAV_REL_TOL, rel_l2
    from wavtokenizer_amd import NAMED_ARCHS
    assert WAV_REL_TOL == 1e-4
    for name in ("hop600", "hop320"):
        m, sd = _model(name)
        orc = OracleWavTokenizer(NAMED_ARCHS[name], sd)
        feats = _feats(m, [5, 40, 120], seed=31)
        wav = m._run_decode_mixed(feats, 120, 0)
        for j, f in enumerate(feats):
            with torch.inference_mode():
                ref = orc.decode(f[None].cpu(), torch.tensor([0]))
            n = m._wave_len(int(f.shape[1]))
            err = rel_l2(wav[j:j + 1, :n].cpu().numpy(), ref.numpy())
            print(f"decode_many oracle {name} L={f.shape[1]}: rel_l2 {err:.3e}")
            assert err < WAV_REL_TOL, (name, j, err)


def test_invalid_length_poisons_the_call(model):
    from wavtokenizer_amd import _capi
    name, m = model
    feats = _feats(m, [10, 20, 30], seed=50)
    for bad in (0, 65):
        wav, plan = _mixed_call(m, feats, 64, 0, 0.0, lengths=[10, bad, 30])
        assert torch.isnan(wav).all(), bad
        bits = ctypes.c_int32()
        _capi.check(_capi.lib.wt_plan_status(plan, ctypes.byref(bits), 1), "wt_plan_status")      # (read and cleared)
        assert bits.value == _capi.WT_STATUS_BIT_LENGTH, (bad, bits.value)
    wav, _plan = _mixed_call(m, feats, 64, 0)             # the plan serves the next call
    _assert_clips(m, wav, feats, [m.decode(f[None], bandwidth_id=torch.tensor([0])) for f in feats])
    _no_status(m)


def test_plan_kinds_and_refusals(model):
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.pretrained import _ptr, _stream_ptr
    name, m = model
    m._ensure_engine()
    lib = _capi.lib
    dev = torch.device("cuda", torch.cuda.current_device())
    mixed, wsm = m._engine.plan(_capi.WT_PLAN_DECODE_MIXED, 2, 40, 0, dev)
    plain, wsp = m._engine.plan(_capi.WT_PLAN_DECODE, 2, 40, 0, dev)
    x = torch.zeros((2, 512, 40), device=dev)
    lens = torch.tensor([40, 7], dtype=torch.int32, device=dev)
    wav = torch.empty((2, m._wave_len(40)), device=dev)
    assert lib.wt_decode(mixed, _ptr(x), 0, _ptr(wav), _ptr(None), _ptr(wsm), _stream_ptr(dev)) == _capi.WT_ERR_INVALID
    assert b"wt_decode_mixed" in lib.wt_last_error()
    assert lib.wt_decode_mixed(plain, _ptr(x), _ptr(lens), 0, _ptr(wav), _ptr(wsp), _stream_ptr(dev)) == _capi.WT_ERR_INVALID
    assert b"mixed-length" in lib.wt_last_error()
    for flag in (_capi.WT_PLAN_FLAG_UNFUSED, _capi.WT_PLAN_FLAG_FP32_GEMM, _capi.WT_PLAN_FLAG_KEEP_STAGES,
                 _capi.WT_PLAN_FLAG_RANGE_REPORT):
        p = ctypes.c_void_p()
        assert lib.wt_plan_create(m._engine.model, _capi.WT_PLAN_DECODE_MIXED, 2, 40, flag, ctypes.byref(p)) == _capi.WT_ERR_INVALID, flag
        assert b"mixed-length" in lib.wt_last_error()
    p = ctypes.c_void_p()
    assert lib.wt_plan_create_ex(m._engine.model, _capi.WT_PLAN_DECODE_MIXED, 2, 40, 0, 1 << _capi.WT_SITE_ATTN,
                                 ctypes.byref(p)) == _capi.WT_ERR_INVALID
    assert b"mixed-length" in lib.wt_last_error()
    assert lib.wt_plan_create(m._engine.model, _capi.WT_PLAN_DECODE, 2, 40, _capi.WT_PLAN_FLAG_MIXED_LENGTH,
                              ctypes.byref(p)) == _capi.WT_ERR_INVALID


def test_fp32_route_falls_back_to_solo_calls():
    from wavtokenizer_amd import _capi
    m, _sd = _model("hop320")
    m.set_gemm_precision("f32")
    feats = _feats(m, [3, 50, 41, 300], seed=4)
    got = m.decode_many(feats, bandwidth_id=torch.tensor([0]))
    for g, f in zip(got, feats):
        assert torch.equal(g, m.decode(f[None], bandwidth_id=torch.tensor([0])))
    assert not [k for k in m._engine.plans if k[0] == _capi.WT_PLAN_DECODE_MIXED]
    m.check_status()
