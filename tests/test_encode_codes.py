"""Tokenising straight from PCM on the GPU (WavTokenizer.encode_codes / encode_codes_many over wt_ingest, wt_encode[_mixed]
without a feature buffer, wt_codes_unpack): every clip's codes are the bits of today's composition - upload, / 32768,
audio.convert_audio, encode_infer - on every route an encode plan takes, and equal the CPU oracle's by the margin rule."""
import random

import numpy as np
import pytest
import torch

from tests import ingest_ref as R

pytestmark = pytest.mark.gpu

BW = torch.tensor([0])
BENCH_RATES = [16000, 22050, 24000, 44100, 48000]


def _load(arch, sd):
    from wavtokenizer_amd import WavTokenizer
    m = WavTokenizer.from_arch(arch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m.eval().to("cuda")


_MODELS = {}


def _cached(name):
    from wavtokenizer_amd import NAMED_ARCHS, synth
    if name not in _MODELS:
        _MODELS[name] = _load(NAMED_ARCHS[name], synth.make_state_dict(NAMED_ARCHS[name], seed=0))
    return _MODELS[name]


@pytest.fixture(scope="module", params=["hop600", "hop320"])
def model(request):
    return request.param, _cached(request.param)


def _no_status(m):
    m.check_status()
    assert not m.fallback_events


def _wav(B, T, seed):
    from wavtokenizer_amd import synth
    return torch.from_numpy(synth.make_clips(B, T, seed=seed)).cuda()


def _encode_plans(m, B, T, mixed=False):
    from wavtokenizer_amd import _capi
    return [(k, p) for k, (p, _ws) in m._engine.plans.items()
            if k[0] == _capi.WT_PLAN_ENCODE and k[1] == B and k[2] == T and bool(k[3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH) == mixed]


# ------------------------------------------------------------------------------------------------ encode_codes
SHAPES = [(2, 9000), (1, 1927)]


def test_encode_codes_is_the_codes_of_encode_infer(model):
    from wavtokenizer_amd import _capi
    name, m = model
    for B, T in SHAPES:
        wav = _wav(B, T, seed=B * 100 + T)
        want = m.encode_infer(wav, bandwidth_id=BW)[1]
        assert want.shape == (1, B, m.arch.frames(T)) and int(want.min()) >= 0
        for rep in range(3):                                 # the second call in a row records the graph, the later ones replay it
            got = m.encode_codes(wav, bandwidth_id=BW)
            assert got.dtype == torch.int64 and got.shape == want.shape and torch.equal(got, want), (name, B, T, rep)
        (key, plan), = _encode_plans(m, B, T)
        assert key[3] & _capi.WT_PLAN_FLAG_GRAPH
        before = _capi.lib.wt_plan_graph_replays(plan)
        assert before >= 2
        for rep in range(3):                                 # encode_infer and encode_codes share the one recording
            assert torch.equal(m.encode_infer(wav, bandwidth_id=BW)[1], want)
            assert torch.equal(m.encode_codes(wav), want)
        assert _capi.lib.wt_plan_graph_replays(plan) == before + 6, (name, B, T)
    _no_status(m)


def test_encode_codes_on_fp32_gemms(model):
    name, m = model
    try:
        m.set_gemm_precision("f32")
        for B, T in SHAPES:
            wav = _wav(B, T, seed=7 + T)
            assert torch.equal(m.encode_codes(wav, bandwidth_id=BW), m.encode_infer(wav, bandwidth_id=BW)[1]), (name, B, T)
    finally:
        m.set_gemm_precision("f16x3")
    _no_status(m)


def test_encode_codes_after_a_range_fallback_of_the_encoder_site():
    """A waveform 10^6 times full scale puts the encoder site on fp32 operands (as tests/test_gpu_parity.py forces it); from then
    on both calls run that route, and encode_codes answers a failing call itself like encode_infer."""
    from wavtokenizer_amd import NAMED_ARCHS, _capi, synth
    arch = NAMED_ARCHS["hop600"]
    sd = synth.make_state_dict(arch, seed=0)
    loud = _wav(2, 9000, seed=77) * 1e6
    m = _load(arch, sd)
    got = m.encode_codes(loud)                               # strict for a small batch: repeated on the fp32 chain
    assert m._fp32_sites == 1 << _capi.WT_SITE_ENCODER, bin(m._fp32_sites)
    assert int(got.min()) >= 0
    assert torch.equal(got, m.encode_infer(loud, bandwidth_id=BW)[1])
    for B, T in SHAPES:
        wav = _wav(B, T, seed=31 + T)
        assert torch.equal(m.encode_codes(wav), m.encode_infer(wav, bandwidth_id=BW)[1]), (B, T)
    # the same codes as a model that reached the site through encode_infer
    m2 = _load(arch, sd)
    want = m2.encode_infer(loud, bandwidth_id=BW)[1]
    assert m2._fp32_sites == m._fp32_sites and torch.equal(got, want)
    for mm in (m, m2):
        with pytest.raises(_capi.WavTokError, match="fallback"):
            mm.check_status()
        _no_status(mm)


# ------------------------------------------------------------------------------------------- encode_codes_many
def _compose(m, clip, rate, layout):
    """The composition encode_codes_many replaces, written out: upload, / 32768, convert_audio, encode_infer."""
    from wavtokenizer_amd import audio
    x = clip.cuda()
    if x.dtype == torch.int16:
        x = x.float() / 32768
    planar = x[None] if layout == "mono" else (x.t() if layout == "interleaved" else x)
    wav = audio.convert_audio(planar.contiguous()[None], rate, R.CODEC_RATE)[0]          # (1, n_out)
    return m.encode_infer(wav, bandwidth_id=BW)[1]


def _random_clips(n, seed, lo=0.05, hi=1.5):
    """[(clip, rate, layout)]: rates of the bench, lo-hi seconds, mixed type, layout and device."""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        rate = rng.choice(BENCH_RATES)
        layout = rng.choice(["mono", "interleaved", "planar"])
        n_in = int(rate * rng.uniform(lo, hi))
        clip = R.make_clip(rate, 1 if layout == "mono" else 2, layout, rng.choice(["f32", "i16"]), n_in, seed=seed * 1000 + i)
        rows.append((clip.cuda() if rng.random() < 0.5 else clip, rate, layout))
    return rows


def _as_layout(rows, channels_last):
    """The clips as one encode_codes_many call takes them: every stereo clip (C, T) or every one (T, C); a clip stored the
    other way round goes in as a transposed view."""
    want = "interleaved" if channels_last else "planar"
    return [c if lay in ("mono", want) else c.t() for c, _sr, lay in rows]


def _check_many(m, rows, want, **kw):
    rates = [r[1] for r in rows]
    for channels_last in (False, True):
        out = m.encode_codes_many(_as_layout(rows, channels_last), sample_rates=rates, channels_last=channels_last, **kw)
        assert len(out) == len(rows)
        for i, (o, w) in enumerate(zip(out, want)):
            assert o.dtype == torch.int64 and o.shape == w.shape == (1, 1, w.shape[-1]), (i, o.shape, w.shape)
            assert torch.equal(o, w), (i, rates[i], rows[i][2], rows[i][0].dtype, rows[i][0].device)
    flat, offs = m.encode_codes_many(_as_layout(rows, False), sample_rates=rates, packed=True, **kw)
    assert offs.device.type == "cpu" and offs.tolist() == np.concatenate([[0], np.cumsum([w.shape[-1] for w in want])]).tolist()
    assert torch.equal(flat, torch.cat([w.reshape(-1) for w in want]))


@pytest.fixture(scope="module")
def mixed_rows():
    return R.table_clips() + _random_clips(20, seed=3)


def test_encode_codes_many_is_the_composition_clip_by_clip(model, mixed_rows):
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.mixed_length import group_clips
    name, m = model
    want = [_compose(m, *r) for r in mixed_rows]
    n_out = [R.out_length(sr, R.planar_f32(c, lay).shape[1]) for c, sr, lay in mixed_rows]
    assert [w.shape[-1] for w in want] == [m.arch.frames(n) for n in n_out]
    m._engine.drop(lambda k: k[0] == _capi.WT_PLAN_ENCODE)
    _check_many(m, mixed_rows, want, bandwidth_id=BW)
    # every group of the policy ran on a mixed-length plan, and only the short clips on plans of their own
    groups, solo = group_clips(n_out, m.arch.hop)
    assert len(solo) == 1 and len(groups) >= 2
    for T_pad, idx in groups:
        assert len(_encode_plans(m, len(idx), T_pad, mixed=True)) == 1, (T_pad, len(idx))
    solo_lengths = {k[2] for k in m._engine.plans if k[0] == _capi.WT_PLAN_ENCODE and not k[3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH}
    assert solo_lengths == {n_out[i] for i in solo}
    _no_status(m)


def test_seventy_clips_split_at_the_group_limit():
    from wavtokenizer_amd.mixed_length import group_clips
    m = _cached("hop600")
    rows = _random_clips(70, seed=11, lo=0.06, hi=0.1)       # 1440 to 2400 samples at the codec rate: one bucket range
    n_out = [R.out_length(sr, R.planar_f32(c, lay).shape[1]) for c, sr, lay in rows]
    groups, solo = group_clips(n_out, 600)
    assert not solo and [len(idx) for _T, idx in groups] == [64, 6]
    want = [_compose(m, *r) for r in rows]
    rates = [r[1] for r in rows]
    out = m.encode_codes_many(_as_layout(rows, False), sample_rates=rates)
    for i, (o, w) in enumerate(zip(out, want)):
        assert torch.equal(o, w), i
    _no_status(m)


def test_on_fp32_gemms_every_clip_goes_solo(mixed_rows):
    from wavtokenizer_amd import _capi
    m = _cached("hop600")
    rows = mixed_rows[:12]
    try:
        m.set_gemm_precision("f32")
        want = [_compose(m, *r) for r in rows]
        m._engine.drop(lambda k: k[0] == _capi.WT_PLAN_ENCODE)
        _check_many(m, rows, want)
        assert not [k for k in m._engine.plans if k[0] == _capi.WT_PLAN_ENCODE and k[3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH]
    finally:
        m.set_gemm_precision("f16x3")
    _no_status(m)


def test_alternating_with_encode_infer_many_replays_one_recording():
    from wavtokenizer_amd import _capi, audio
    m = _cached("hop600")
    from wavtokenizer_amd.mixed_length import group_clips
    rows = [r for r in R.table_clips() if R.out_length(r[1], R.planar_f32(r[0], r[2]).shape[1]) >= 8000]
    rows.append((R.make_clip(R.CODEC_RATE, 1, "mono", "i16", 9001, seed=40), R.CODEC_RATE, "mono"))
    groups, solo = group_clips([R.out_length(r[1], R.planar_f32(r[0], r[2]).shape[1]) for r in rows], 600)
    assert len(rows) == 4 and not solo and [len(idx) for _T, idx in groups] == [4]      # one group, graph-replayed
    rates = [r[1] for r in rows]
    clips = _as_layout(rows, False)
    wavs = [audio.convert_audio(R.planar_f32(c.cuda(), lay).contiguous()[None], sr, R.CODEC_RATE)[0, 0] for c, sr, lay in rows]
    want = [c for _f, c in m.encode_infer_many(wavs, bandwidth_id=BW)]
    replays = []
    for rep in range(5):
        got = m.encode_codes_many(clips, sample_rates=rates)
        again = [c for _f, c in m.encode_infer_many(wavs, bandwidth_id=BW)]
        for g, a, w in zip(got, again, want):
            assert torch.equal(g, w) and torch.equal(a, w), rep
        plans = [p for k, p in [(k, p) for k, (p, _ws) in m._engine.plans.items()]
                 if k[0] == _capi.WT_PLAN_ENCODE and k[1] == 4 and k[3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH and k[3] & _capi.WT_PLAN_FLAG_GRAPH]
        assert len(plans) == 1                               # one plan, one staging set, one recording for both callers
        replays.append(_capi.lib.wt_plan_graph_replays(plans[0]))
    # (the call that made `want` remembered the key or replayed already) both calls of every round replay: nothing records again
    assert [b - a for a, b in zip(replays, replays[1:])] == [2, 2, 2, 2], replays
    _no_status(m)


def test_pinned_and_pageable_host_clips():
    """Rows of a pinned batch, a prefix of one, a pinned stereo clip and a pageable clip in one call: the composition's codes."""
    m = _cached("hop600")
    host = torch.stack([R.make_clip(R.CODEC_RATE, 1, "mono", "i16", 24000, seed=60 + i) for i in range(6)]).pin_memory()
    stereo = R.make_clip(44100, 2, "planar", "f32", 40000, seed=70).pin_memory()
    loose = R.make_clip(16000, 1, "mono", "f32", 15000, seed=71)                          # pageable
    clips = [host[0], host[1], loose, host[2], stereo, host[3], host[4], host[5][:20000]]
    rates = [R.CODEC_RATE, R.CODEC_RATE, 16000, R.CODEC_RATE, 44100, R.CODEC_RATE, R.CODEC_RATE, R.CODEC_RATE]
    want = [_compose(m, c, sr, "mono" if c.dim() == 1 else "planar") for c, sr in zip(clips, rates)]
    for i, (g, w) in enumerate(zip(m.encode_codes_many(clips, sample_rates=rates), want)):
        assert torch.equal(g, w), i
    _no_status(m)


def test_no_feature_tensor_on_the_direct_path(mixed_rows):
    """Above the graph limit of 16 clips the features argument that reaches wt_encode_mixed / wt_encode is null; a graph plan
    keeps passing its staging buffer."""
    from wavtokenizer_amd import _capi
    m = _cached("hop600")
    seen = []

    def wrap(name, feat_arg):
        real = getattr(_capi.lib, name)

        def entry(*args):
            seen.append((name, args[feat_arg].value))
            return real(*args)
        setattr(_capi.lib, name, entry)
        return real

    real_mixed, real_plain = wrap("wt_encode_mixed", 3), wrap("wt_encode", 2)
    try:
        big = _random_clips(20, seed=3, lo=0.06, hi=0.1)     # one group of 20
        m.encode_codes_many(_as_layout(big, False), sample_rates=[r[1] for r in big])
        assert seen and all(n == "wt_encode_mixed" and not p for n, p in seen), seen
        del seen[:]
        m.encode_codes_many(_as_layout(big[:5], False), sample_rates=[r[1] for r in big[:5]])
        assert [n for n, _p in seen] == ["wt_encode_mixed"] and seen[0][1]
        del seen[:]
        m.encode_codes(_wav(17, 1927, seed=4))
        assert seen == [("wt_encode", None)]
        del seen[:]
        m.encode_infer(_wav(17, 1927, seed=4), bandwidth_id=BW)
        assert [n for n, _p in seen] == ["wt_encode"] and seen[0][1]
    finally:
        _capi.lib.wt_encode_mixed, _capi.lib.wt_encode = real_mixed, real_plain
    _no_status(m)


# ----------------------------------------------------------------------------------------------- against the oracle
def test_codes_against_the_cpu_oracle():
    """oracle.audio_ref.convert_audio, then the oracle's encode_infer with its top-2 margin: codes equal, or differ only at a
    near tie of the oracle itself (tests.util.check_codes); at most 2 % of the compared frames may be such ties."""
    from oracle.audio_ref import convert_audio
    from oracle.cpu_ref import OracleWavTokenizer
    from tests.util import NEAR_TIE_MARGIN, check_codes
    from wavtokenizer_amd import NAMED_ARCHS, synth
    assert NEAR_TIE_MARGIN == 0.02
    arch = NAMED_ARCHS["hop600"]
    orc = OracleWavTokenizer(arch, synth.make_state_dict(arch, seed=0))
    m = _cached("hop600")
    rows = [r for r in R.table_clips() if R.out_length(r[1], R.planar_f32(r[0], r[2]).shape[1]) >= 1024]
    assert len(rows) == 7
    got = m.encode_codes_many(_as_layout(rows, False), sample_rates=[r[1] for r in rows])
    frames = ties = flips = 0
    for (clip, rate, layout), g in zip(rows, got):
        wav = convert_audio(R.planar_f32(clip, layout).numpy(), rate, R.CODEC_RATE)          # (1, n_out)
        taps = {}
        with torch.inference_mode():
            _f, co = orc.encode_infer(torch.from_numpy(np.ascontiguousarray(wav)), BW, taps)
        margin = taps["vq.margin"].numpy()
        flips += check_codes(g.cpu().numpy(), co.numpy(), margin, f"{rate} Hz {layout}")
        frames += co.numel()
        ties += int((margin.reshape(-1) < NEAR_TIE_MARGIN).sum())
    print(f"encode_codes_many against the oracle: {frames} frames, {ties} near ties in the oracle, {flips} flips")
    assert frames == 92 and ties <= 0.02 * frames, (frames, ties)
    _no_status(m)
