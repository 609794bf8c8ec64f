"""Mixed-length encode (WT_PLAN_FLAG_MIXED_LENGTH, wt_encode_mixed, WavTokenizer.encode_infer_many) on the GPU: every clip's
codes and features are the bits a call of its own length returns, whatever the batch, order, grouping or padding."""
import ctypes
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(name):
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth
    arch = NAMED_ARCHS[name]
    sd = synth.make_state_dict(arch, seed=321)
    m = WavTokenizer.from_arch(arch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m.eval().to("cuda")


@pytest.fixture(scope="module", params=["hop600", "hop320"])
def model(request):
    return request.param, _model(request.param)


def _clips(lengths, seed):
    from wavtokenizer_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for i, T in enumerate(lengths):
        x = synth.make_clips(1, int(T), seed=seed + i)[0] * np.float32(0.5 + rng.random())
        out.append(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    return out


def _solo(m, wavs):
    return [m.encode_infer(w[None], bandwidth_id=torch.tensor([0])) for w in wavs]


def _assert_same(got, ref):
    assert len(got) == len(ref)
    for i, ((f, c), (rf, rc)) in enumerate(zip(got, ref)):
        assert f.shape == rf.shape and c.shape == rc.shape, (i, f.shape, rf.shape, c.shape, rc.shape)
        assert torch.equal(c, rc), i
        assert torch.equal(f, rf), i


def _encode_many_on_the_mixed_route(m, wavs, **kw):
    """encode_infer_many, checked to have run every clip of MIN_CLIP samples or more through mixed-length plans: one plan per
    group of the grouping policy, and no one-clip encode plan for any of those lengths (the per-clip fallback makes them)."""
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.mixed_length import MIN_CLIP, group_clips
    m._ensure_engine()
    m._engine.drop(lambda k: k[0] == _capi.WT_PLAN_ENCODE)
    out = m.encode_infer_many(wavs, **kw)
    lengths = [int(w.shape[0]) for w in wavs]
    groups, solo = group_clips(lengths, m.arch.hop)
    keys = _mixed_plans(m)
    for T_pad, idx in groups:
        assert any(k[1] == len(idx) and k[2] == T_pad for k in keys), (T_pad, len(idx), keys)
    plain = [k for k in m._engine.plans if k[0] == _capi.WT_PLAN_ENCODE and not k[3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH]
    assert sorted(k[2] for k in plain) == sorted(set(lengths[i] for i in solo)), plain
    assert all(lengths[i] < MIN_CLIP for i in solo)
    return out


def _edge_lengths(name):
    hop = 600 if name == "hop600" else 320
    R = 4 if name == "hop600" else 2                   # stride of the fused stage-1 down conv
    opt = (126 - 2 * R) // R + 1                       # its output frames per tile
    k = -(-1100 // hop)
    L = [1024, 1025,                                   # the shortest clips a mixed plan takes
         k * hop - 1, k * hop, k * hop + 1,            # around a multiple of the hop
         R * opt * 20 + 7, R * opt * 33 + R * opt - 3]  # the last stage-1 tile shifted to end at the clip
    if name == "hop600":
        L += [1200, 1201, 1800]                        # L = 2, 3, 3: the final conv's short-input reflect rule
    L += [72000, 720000, 700, 1023]                    # 3 s, 30 s, two clips below the mixed plan's minimum (fallback)
    return L


def test_encode_infer_many_matches_solo_calls(model):
    name, m = model
    wavs = _clips(_edge_lengths(name), seed=100)
    got = _encode_many_on_the_mixed_route(m, wavs, bandwidth_id=torch.tensor([0]))
    _assert_same(got, _solo(m, wavs))
    hop = m.arch.hop
    for w, (f, c) in zip(wavs, got):
        assert f.shape == (1, 512, -(-w.shape[0] // hop)) and c.shape == (1, 1, f.shape[2])
    m.check_status()
    assert not m.fallback_events


def test_order_and_grouping_do_not_matter(model):
    name, m = model
    rng = random.Random(5)
    lengths = [rng.choice([1024, 1500, 2047, 4800, 9601, 24000]) for _ in range(130)]      # > 128 clips: several calls
    from wavtokenizer_amd.mixed_length import group_clips
    groups, solo = group_clips(lengths, m.arch.hop)
    assert len(groups) >= 2 and not solo
    wavs = _clips(lengths, seed=900)
    got = _encode_many_on_the_mixed_route(m, wavs)
    ref = _solo(m, wavs)
    _assert_same(got, ref)
    perm = list(range(len(wavs)))
    rng.shuffle(perm)
    got_p = _encode_many_on_the_mixed_route(m, [wavs[i] for i in perm])
    _assert_same(got_p, [ref[i] for i in perm])
    m.check_status()


def _mixed_plans(m):
    from wavtokenizer_amd import _capi
    return [k for k in m._engine.plans if k[0] == _capi.WT_PLAN_ENCODE and k[3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH]


def test_plans_and_graphs_are_reused(model):
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.mixed_length import bucket_length
    name, m = model
    hop = m.arch.hop
    m._engine.drop(lambda k: k[3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH)
    top = bucket_length(40000, hop)
    sets = [[40000, 30001, 25000, 39000], [top - 1, 27000, 33333, 35555], [38000, 39999, 26000, 23000]]
    assert len({bucket_length(max(s), hop) for s in sets}) == 1
    replays = []
    for i, lengths in enumerate(sets):
        wavs = _clips(lengths, seed=3000 + 10 * i)
        _assert_same(m.encode_infer_many(wavs), _solo(m, wavs))
        keys = _mixed_plans(m)
        assert len(keys) == 1, keys                              # one plan for the bucket
        replays.append(_capi.lib.wt_plan_graph_replays(m._engine.plans[keys[0]][0]))
    assert replays[2] > replays[1] >= 1, replays                 # the group of 4 replays its graph with new lengths
    m.check_status()


def _mixed_call(m, B, T_pad, wav, lengths, emb=False):
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.pretrained import _ptr, _stream_ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    plan, ws = m._engine.plan(_capi.WT_PLAN_ENCODE, B, T_pad, _capi.WT_PLAN_FLAG_MIXED_LENGTH, dev)
    L = m.arch.frames(T_pad)
    feats = torch.full((B, 512, L), 7.0, device=dev)
    codes = torch.full((1, B, L), 7, dtype=torch.int64, device=dev)
    e = torch.full((B, 512, L), 7.0, device=dev) if emb else None
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    _capi.check(_capi.lib.wt_encode_mixed(plan, _ptr(wav), _ptr(lens), _ptr(feats), _ptr(codes), _ptr(e), _ptr(ws),
                                          _stream_ptr(dev)), "wt_encode_mixed")
    torch.cuda.synchronize()
    bits = ctypes.c_int32()
    _capi.check(_capi.lib.wt_plan_status(plan, ctypes.byref(bits), 0), "wt_plan_status")
    return feats, codes, e, bits.value, plan


def test_padding_samples_are_never_read(model):
    name, m = model
    lengths = [5000, 1024, 12345]
    T_pad = 13000
    wavs = _clips(lengths, seed=55)
    outs = []
    for fill in (0.0, float("nan"), 1e30):
        wav = torch.full((3, T_pad), fill, device="cuda")
        for j, w in enumerate(wavs):
            wav[j, :w.shape[0]] = w
        f, c, e, bits, _plan = _mixed_call(m, 3, T_pad, wav, lengths, emb=True)
        assert bits == 0
        outs.append((f, c, e))
    for f, c, e in outs[1:]:
        assert torch.equal(f, outs[0][0]) and torch.equal(c, outs[0][1]) and torch.equal(e, outs[0][2])
    f, c, e = outs[0]
    hop = m.arch.hop
    for j, w in enumerate(wavs):
        L = -(-lengths[j] // hop)
        with torch.inference_mode():              # (as encode_infer calls it: the graph plans' staging tensors are shared)
            rf, rc, re_ = m._run_encode(w[None], want_emb=True)
        assert torch.equal(f[j:j + 1, :, :L], rf) and torch.equal(c[:, j:j + 1, :L], rc) and torch.equal(e[j:j + 1, :, :L], re_)
        assert (c[0, j, L:] == -1).all() and (f[j, :, L:] == 0).all() and (e[j, :, L:] == 0).all()
    m.check_status()
    assert not m.fallback_events


def test_invalid_length_poisons_only_its_own_row(model):
    from wavtokenizer_amd import _capi
    name, m = model
    T_pad = 9000
    base = [4000, 1024, 9000, 7777]
    wavs = _clips(base, seed=77)
    ref = _solo(m, wavs)
    hop = m.arch.hop
    for bad in (0, T_pad + 1, 1023):
        wav = torch.zeros((5, T_pad), device="cuda")
        lengths = [base[0], bad, base[1], base[2], base[3]]
        for j, w in zip([0, 2, 3, 4], wavs):
            wav[j, :w.shape[0]] = w
        wav[1] = 1e30                                   # an invalid clip reads nothing either
        f, c, _e, bits, _plan = _mixed_call(m, 5, T_pad, wav, lengths)
        assert bits == 0, bad
        assert (c[0, 1] == -1).all() and torch.isnan(f[1]).all()
        for j, (rf, rc) in zip([0, 2, 3, 4], ref):
            L = rf.shape[2]
            assert torch.equal(f[j:j + 1, :, :L], rf) and torch.equal(c[:, j:j + 1, :L], rc)
    bits = ctypes.c_int32()
    _capi.check(_capi.lib.wt_model_status(m._engine.model, ctypes.byref(bits), 0), "wt_model_status")
    assert bits.value == 0
    m.check_status()


def test_plan_kinds_and_refusals(model):
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.mixed_length import MIN_CLIP
    from wavtokenizer_amd.pretrained import _ptr, _stream_ptr
    name, m = model
    m._ensure_engine()
    lib = _capi.lib
    dev = torch.device("cuda", torch.cuda.current_device())
    mixed, wsm = m._engine.plan(_capi.WT_PLAN_ENCODE, 2, 4096, _capi.WT_PLAN_FLAG_MIXED_LENGTH, dev)
    plain, wsp = m._engine.plan(_capi.WT_PLAN_ENCODE, 2, 4096, 0, dev)
    assert lib.wt_plan_min_clip_length(mixed) == MIN_CLIP and lib.wt_plan_min_clip_length(plain) == 0
    wav = torch.zeros((2, 4096), device=dev)
    lens = torch.tensor([4096, 2000], dtype=torch.int32, device=dev)
    L = m.arch.frames(4096)
    feats = torch.empty((2, 512, L), device=dev)
    codes = torch.empty((1, 2, L), dtype=torch.int64, device=dev)
    assert lib.wt_encode(mixed, _ptr(wav), _ptr(feats), _ptr(codes), _ptr(None), _ptr(wsm), _stream_ptr(dev)) == _capi.WT_ERR_INVALID
    assert b"wt_encode_mixed" in lib.wt_last_error()
    assert lib.wt_encode_mixed(plain, _ptr(wav), _ptr(lens), _ptr(feats), _ptr(codes), _ptr(None), _ptr(wsp), _stream_ptr(dev)) \
        == _capi.WT_ERR_INVALID
    assert b"mixed-length" in lib.wt_last_error()
    for flag in (_capi.WT_PLAN_FLAG_UNFUSED, _capi.WT_PLAN_FLAG_FP32_GEMM, _capi.WT_PLAN_FLAG_KEEP_STAGES,
                 _capi.WT_PLAN_FLAG_RANGE_REPORT):
        p = ctypes.c_void_p()
        assert lib.wt_plan_create(m._engine.model, _capi.WT_PLAN_ENCODE, 2, 4096, _capi.WT_PLAN_FLAG_MIXED_LENGTH | flag,
                                  ctypes.byref(p)) == _capi.WT_ERR_INVALID, flag
        assert b"mixed-length" in lib.wt_last_error()
    p = ctypes.c_void_p()
    assert lib.wt_plan_create_ex(m._engine.model, _capi.WT_PLAN_ENCODE, 2, 4096, _capi.WT_PLAN_FLAG_MIXED_LENGTH,
                                 1 << _capi.WT_SITE_ENCODER, ctypes.byref(p)) == _capi.WT_ERR_INVALID
    assert lib.wt_plan_create(m._engine.model, _capi.WT_PLAN_ENCODE, 2, 1000, _capi.WT_PLAN_FLAG_MIXED_LENGTH,
                              ctypes.byref(p)) == _capi.WT_ERR_INVALID
    assert lib.wt_plan_create(m._engine.model, _capi.WT_PLAN_DECODE, 2, 40, _capi.WT_PLAN_FLAG_MIXED_LENGTH,
                              ctypes.byref(p)) == _capi.WT_ERR_INVALID


def test_fp32_route_falls_back_to_solo_calls():
    name = "hop320"
    m = _model(name)
    m.set_gemm_precision("f32")
    wavs = _clips([1024, 3000, 1500, 800], seed=4)
    got = m.encode_infer_many(wavs)
    _assert_same(got, _solo(m, wavs))
    assert not _mixed_plans(m)
    m.check_status()


def test_encoder_output_is_batch_invariant_up_to_the_group_limit():
    """The grouping policy's 64-clip limit rests on this: with 64 clips per call (the persistent LSTM) every clip's encoder
    output, before quantisation, is the bits of a one-clip call."""
    from wavtokenizer_amd import synth
    from wavtokenizer_amd.mixed_length import MAX_GROUP
    assert MAX_GROUP == 64
    m = _model("hop600")
    m.set_graph_max_clips(0)
    wav = torch.from_numpy(synth.make_clips(MAX_GROUP, 120000, seed=3)).cuda()
    with torch.inference_mode():
        emb = m._run_encode(wav, want_emb=True)[2]
        for i in range(0, MAX_GROUP, 9):
            assert torch.equal(emb[i:i + 1], m._run_encode(wav[i:i + 1], want_emb=True)[2]), i
    assert m.persistent_lstm
    m.check_status()
