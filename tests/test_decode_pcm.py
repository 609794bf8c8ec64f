"""Synthesising straight to PCM (WavTokenizer.decode_pcm / decode_pcm_many: decode from codes, then one ragged emit launch,
wt_emit) on the GPU: every clip is, on each channel, the bits of the composition it replaces, decode_codes ->
audio.convert_audio -> audio.to_pcm16 of that clip alone, whatever the other clips, their order, the grouping, the GEMM mode
and the route the decoder takes."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import emit_ref as R

pytestmark = pytest.mark.gpu

FRAMES = [1, 2, 3, 7, 40, 41, 75]
RATES = [8000, 16000, 22050, 24000, 44100, 48000]
FORMATS = [dict(channels=2, dtype=torch.int16, channels_last=True),          # int16 stereo interleaved
           dict(channels=1, dtype=torch.float32, channels_last=False)]        # fp32 mono planar
LIMIT = 0.5              # the synthetic decoder's waveforms peak near +-0.9: a limit they pass on both sides (asserted below)

_MODELS = {}


def _cached(name):
    """hop600 / hop320 with synthetic weights (as tests/test_decode_codes.py); "center": hop600 with the ISTFT's center padding."""
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth
    if name not in _MODELS:
        arch = dataclasses.replace(NAMED_ARCHS["hop600"], padding="center") if name == "center" else NAMED_ARCHS[name]
        m = WavTokenizer.from_arch(arch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, seed=321).items()}, strict=False)
        _MODELS[name] = m.eval().to("cuda")
    return _MODELS[name]


def _clips(m, frames, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, m.arch.vq_bins, size=(1, int(L)))).cuda() for L in frames]


def _rates(n):
    return [RATES[i % len(RATES)] for i in range(n)]


def _bw(i=0):
    return torch.tensor([i])


def _no_status(m):
    m.check_status()
    assert not m.fallback_events


_WANT = {}


def _want(m, key, clips, rates, fmt, limit=LIMIT):
    """The composition of every clip, computed once per (model, mode, clip set, format) and shared, never modified."""
    k = (id(m), key, fmt["channels"], fmt["dtype"], fmt["channels_last"], limit)
    if k not in _WANT:
        _WANT[k] = [R.pcm_composition(m, c, sr, fmt["channels"], fmt["dtype"], fmt["channels_last"], limit, _bw()) for c, sr in zip(clips, rates)]
    return _WANT[k]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape)
        assert torch.equal(g, w), (what, i, int((g != w).sum()))


@pytest.fixture(scope="module")
def model600():
    return _cached("hop600")


@pytest.fixture(scope="module")
def clips600(model600):
    return _clips(model600, FRAMES, seed=7)


@pytest.mark.parametrize("fmt", FORMATS, ids=["i16-stereo-interleaved", "f32-mono-planar"])
def test_decode_pcm_many_is_the_bits_of_the_composition(model600, clips600, fmt):
    m, rates = model600, _rates(len(FRAMES))
    want = _want(m, "f16x3", clips600, rates, fmt)
    got = m.decode_pcm_many(clips600, sample_rates=rates, limit=LIMIT, bandwidth_id=_bw(), **fmt)
    for g, L, sr in zip(got, FRAMES, rates):
        n = -(-sr * 600 * L // 24000)
        assert tuple(g.shape) == ((n, 2) if fmt["channels_last"] else (1, n))
    _assert_same(got, want, "many")
    if fmt["dtype"] == torch.int16:
        top = int(LIMIT * 32768 + 0.5)                       # (0.5 * 32768)
        assert max(int(g.max()) for g in got) == top and min(int(g.min()) for g in got) == -top      # the clamp is hit
        assert all(torch.equal(g[:, 0], g[:, 1]) for g in got)
    assert got[0].untyped_storage().data_ptr() == got[-1].untyped_storage().data_ptr()               # views of one flat tensor
    _no_status(m)


def test_packed_offsets_and_input_order(model600, clips600):
    m, rates, fmt = model600, _rates(len(FRAMES)), FORMATS[0]
    want = _want(m, "f16x3", clips600, rates, fmt)
    flat, offs = m.decode_pcm_many(clips600, sample_rates=rates, limit=LIMIT, packed=True, bandwidth_id=_bw(), **fmt)
    n_out = [w.shape[0] for w in want]
    assert offs.device.type == "cpu" and offs.tolist() == [2 * sum(n_out[:i]) for i in range(len(n_out) + 1)]
    assert flat.shape == (offs[-1],) and flat.dtype == torch.int16 and flat.is_cuda
    _assert_same([flat[offs[i]:offs[i + 1]].view(-1, 2) for i in range(len(n_out))], want, "packed")
    back = m.decode_pcm_many(clips600[::-1], sample_rates=rates[::-1], limit=LIMIT, bandwidth_id=_bw(), **fmt)
    _assert_same(back[::-1], want, "reversed")
    # one rate for all, the (K, 1, L) form, and the default: the codec rate, mono int16, limit 0.99
    one = m.decode_pcm_many([c[:, None, :] for c in clips600[3:6]], sample_rates=44100, dtype=torch.float32, bandwidth_id=_bw())
    _assert_same(one, [R.pcm_composition(m, c, 44100, 1, torch.float32, False, 0.99, _bw()) for c in clips600[3:6]], "one rate")
    # a channel count per clip in one call
    chans = [1 + i % 2 for i in range(len(FRAMES))]
    mix = m.decode_pcm_many(clips600, sample_rates=rates, channels=chans, channels_last=True, limit=LIMIT, bandwidth_id=_bw())
    _assert_same(mix, [w if c == 2 else w[:, :1].contiguous() for w, c in zip(want, chans)], "channels per clip")
    dflt = m.decode_pcm_many(clips600[4:6], bandwidth_id=_bw())
    _assert_same(dflt, [R.pcm_composition(m, c, 24000, 1, torch.int16, False, 0.99, _bw()) for c in clips600[4:6]], "default")
    _no_status(m)


def test_host_output_is_the_device_result_in_pinned_memory(model600, clips600):
    m, rates = model600, _rates(len(FRAMES))
    for fmt in FORMATS:
        want = _want(m, "f16x3", clips600, rates, fmt)
        flat, offs = m.decode_pcm_many(clips600, sample_rates=rates, limit=LIMIT, packed=True, device="cpu", bandwidth_id=_bw(), **fmt)
        assert flat.device.type == "cpu" and flat.is_pinned() and flat.dtype == fmt["dtype"]
        assert torch.equal(flat, torch.cat([w.reshape(-1) for w in want]).cpu())         # (no wait here: the call has waited)
        got = m.decode_pcm_many(clips600, sample_rates=rates, limit=LIMIT, device="cpu", bandwidth_id=_bw(), **fmt)
        assert all(g.device.type == "cpu" for g in got)
        _assert_same(got, [w.cpu() for w in want], "host")


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "direct"])
def test_decode_pcm_is_the_bits_of_the_composition(model600, graph):
    from wavtokenizer_amd import _capi
    m = model600
    rng = np.random.default_rng(11)
    try:
        m.set_graph_max_clips(16 if graph else 0)
        for B, L, rate, fmt in ((1, 41, 48000, FORMATS[0]), (3, 40, 22050, FORMATS[0]), (3, 7, 16000, FORMATS[1]),
                                (1, 75, 24000, dict(channels=2, dtype=torch.float32, channels_last=False))):
            codes = torch.from_numpy(rng.integers(0, m.arch.vq_bins, size=(1, B, L))).cuda()
            want = torch.stack([R.pcm_composition(m, codes[:, b], rate, fmt["channels"], fmt["dtype"], fmt["channels_last"], LIMIT, _bw())
                                for b in range(B)])
            for _rep in range(3 if graph else 1):            # the second call records the graph, it and the third replay it
                got = m.decode_pcm(codes, sample_rate=rate, limit=LIMIT, bandwidth_id=_bw(), **fmt)
                n = -(-rate * 600 * L // 24000)
                assert tuple(got.shape) == ((B, n, fmt["channels"]) if fmt["channels_last"] else (B, fmt["channels"], n))
                assert got.dtype == want.dtype and torch.equal(got, want), (B, L, rate, _rep)
            if B == 1:                                       # the (K, L) form
                assert torch.equal(m.decode_pcm(codes[:, 0], sample_rate=rate, limit=LIMIT, bandwidth_id=_bw(), **fmt), want)
            keys = [k for k in m._engine.plans if k[0] == _capi.WT_PLAN_DECODE_CODES and k[1] == B and k[2] == L]
            assert any(bool(k[3] & _capi.WT_PLAN_FLAG_GRAPH) == graph for k in keys)
    finally:
        m.set_graph_max_clips(16)
    _no_status(m)


def test_hop320():
    m = _cached("hop320")
    frames = [2, 9, 10, 33]
    clips, rates = _clips(m, frames, seed=3), [44100, 8000, 48000, 22050]
    for fmt in FORMATS:
        got = m.decode_pcm_many(clips, sample_rates=rates, limit=LIMIT, bandwidth_id=_bw(), **fmt)
        assert [g.shape[0 if fmt["channels_last"] else 1] for g in got] == [-(-sr * 320 * L // 24000) for sr, L in zip(rates, frames)]
        _assert_same(got, _want(m, "f16x3", clips, rates, fmt), "hop320")
    _no_status(m)


def test_center_padding_and_its_one_frame_clip():
    m = _cached("center")
    frames = [2, 5, 6, 40]
    clips, rates, fmt = _clips(m, frames, seed=5), [16000, 44100, 24000, 48000], FORMATS[0]
    got = m.decode_pcm_many(clips, sample_rates=rates, limit=LIMIT, bandwidth_id=_bw(), **fmt)
    assert [g.shape[0] for g in got] == [-(-sr * 600 * (L - 1) // 24000) for sr, L in zip(rates, frames)]      # wave_len = (L - 1) * hop
    _assert_same(got, _want(m, "f16x3", clips, rates, fmt), "center")
    one = _clips(m, [1], seed=6)[0]
    with pytest.raises(Exception) as solo:                   # a one-frame 'center' clip has no samples: decode_codes refuses it
        m.decode_codes(one, bandwidth_id=_bw())
    with pytest.raises(type(solo.value)):
        m.decode_pcm_many(clips + [one], sample_rates=rates + [24000], limit=LIMIT, bandwidth_id=_bw(), **fmt)
    with pytest.raises(type(solo.value)):
        m.decode_pcm(one, limit=LIMIT, bandwidth_id=_bw())
    _assert_same(m.decode_pcm_many(clips, sample_rates=rates, limit=LIMIT, bandwidth_id=_bw(), **fmt), got, "center again")
    _no_status(m)


def test_f16_mode_gives_the_compositions_bits_under_that_mode(model600, clips600):
    m, rates = model600, _rates(len(FRAMES))
    try:
        m.set_gemm_precision("f16")
        half = {i: _want(m, "f16", clips600, rates, fmt) for i, fmt in enumerate(FORMATS)}
        for i, fmt in enumerate(FORMATS):
            _assert_same(m.decode_pcm_many(clips600, sample_rates=rates, limit=LIMIT, bandwidth_id=_bw(), **fmt), half[i], "f16")
    finally:
        m.set_gemm_precision("f16x3")
    full = _want(m, "f16x3", clips600, rates, FORMATS[1])
    assert not all(torch.equal(a, b) for a, b in zip(half[1], full))          # (the mode does change the waveform)
    _no_status(m)


def test_off_the_mixed_route_every_clip_goes_solo(model600, clips600):
    m, rates = model600, _rates(len(FRAMES))
    calls = []
    real = m._decode_pcm_solo
    try:
        m.set_gemm_precision("f32")
        m._decode_pcm_solo = lambda specs, *a: (calls.append([sp.frames for sp in specs]), real(specs, *a))[1]
        for fmt in FORMATS:
            want = _want(m, "f32", clips600, rates, fmt)
            _assert_same(m.decode_pcm_many(clips600, sample_rates=rates, limit=LIMIT, bandwidth_id=_bw(), **fmt), want, "f32")
        assert calls == [FRAMES, FRAMES]                     # every clip, in input order, in one solo pass per call
    finally:
        del m._decode_pcm_solo
        m.set_gemm_precision("f16x3")
    _no_status(m)


def test_a_bad_code_raises_under_sync(model600, clips600):
    from wavtokenizer_amd import _capi
    m = model600
    bad = [c.clone() for c in clips600[3:6]]
    bad[1][0, 3] = m.arch.vq_bins
    assert m._check_codes == "sync"
    try:
        with pytest.raises(IndexError, match="index out of range in self"):
            m.decode_pcm_many(bad, sample_rates=16000, bandwidth_id=_bw())
        with pytest.raises(IndexError, match="index out of range in self"):
            m.decode_pcm(bad[1], sample_rate=16000, bandwidth_id=_bw())
        got = m.decode_pcm_many(clips600[3:6], sample_rates=16000, dtype=torch.float32, bandwidth_id=_bw())      # (the flag was consumed)
        _assert_same(got, [R.pcm_composition(m, c, 16000, 1, torch.float32, False, 0.99, _bw()) for c in clips600[3:6]], "after")
    finally:
        _capi.lib.wt_model_take_bad_codes(m._engine.model)
    _no_status(m)
