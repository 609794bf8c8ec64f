"""Long recordings in batched segments on the GPU (WavTokenizer.encode_codes_segmented(_many) / decode_pcm_segmented(_many)): every
segment's codes are the bits of encode_codes on that cut of the resampled recording, every synthesised recording is the bits of
the composition it replaces (decode_codes per segment -> audio.linear_overlap_add -> audio.convert_audio -> audio.to_pcm16),
whatever the other recordings, their order, the grouping and the GEMM mode; and the round trip stays within the project's
waveform tolerance of the oracle's segment loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S, STRIDE = 4800, 3600                                       # 8 frames at hop 600
# samples at 24 kHz, source rate, source form
RECORDINGS = [(4800, 24000, "f32-mono-gpu"),
              (4801, 44100, "i16-stereo-cpu"),
              (3000, 16000, "f32-mono-cpu"),
              (8400, 16000, "f32-stereo-gpu"),
              (7200, 24000, "f32-mono-gpu"),
              (500, 44100, "i16-stereo-cpu"),                # below MIN_CLIP: the solo route
              (3601, 44100, "i16-stereo-cpu"),               # a one-sample tail
              (3600 * 69 + 4800, 24000, "f32-mono-gpu")]     # 70 full segments and a tail: crosses the 64-clip group edge
DEEP = (12000, 1500)                                         # one more recording at stride 1500: four deep, three short tails
FORMATS = [dict(channels=2, dtype=torch.int16, channels_last=True),          # int16 stereo interleaved
           dict(channels=1, dtype=torch.float32, channels_last=False)]        # fp32 mono planar
LIMIT = 0.25             # the synthetic decoder's waveforms peak well above it: a limit they pass on both sides (asserted below)

_MODELS = {}


def _cached(name):
    """hop600 with synthetic weights: "seed321" as tests/test_decode_pcm.py, "golden" the weights the oracle fixtures use."""
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth
    from tests.util import synth_state_dict
    if name not in _MODELS:
        arch = NAMED_ARCHS["hop600"]
        sd = synth.make_state_dict(arch, seed=321) if name == "seed321" else synth_state_dict("hop600")
        m = WavTokenizer.from_arch(arch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        _MODELS[name] = m.eval().to("cuda")
    return _MODELS[name]


def _bw(i=0):
    return torch.tensor([i])


def _no_status(m):
    m.check_status()
    assert not m.fallback_events


def _source(n24, rate, form, seed):
    """(clip as the caller holds it, the same clip as planar fp32 on the GPU): the shortest source whose resampled length is n24."""
    from wavtokenizer_amd import synth
    n = next(k for k in range(max(1, n24 * rate // 24000 - 2), n24 * rate // 24000 + 3) if -(-24000 * k // rate) == n24)
    x = synth.make_clips(2, n, seed=seed, sample_rate=rate)                                  # (2, n) fp32
    if form.startswith("i16-stereo"):
        q = torch.from_numpy(np.rint(x * 32767.0).astype(np.int16))
        return q.t().contiguous(), (q.float() / 32768.0).cuda()                             # interleaved (n, 2) on the CPU
    if form.startswith("f32-stereo"):
        t = torch.from_numpy(x).cuda()
        return t.t().contiguous(), t                                                        # interleaved (n, 2) on the GPU
    t = torch.from_numpy(x[0])
    return (t.cuda() if form.endswith("gpu") else t), t.cuda()[None]


@pytest.fixture(scope="module")
def model():
    return _cached("seed321")


@pytest.fixture(scope="module")
def sources():
    return [_source(n24, rate, form, seed=60 + j) for j, (n24, rate, form) in enumerate(RECORDINGS)]


@pytest.fixture(scope="module")
def want_codes(model, sources):
    """Per recording the codes of every segment by hand: resample first, cut second, encode_codes per cut.  Computed once, shared."""
    from wavtokenizer_amd import audio
    from wavtokenizer_amd.segmented import segment_plan
    out = []
    for (n24, rate, _form), (_clip, planar) in zip(RECORDINGS, sources):
        W = audio.convert_audio(planar, rate, 24000, 1)                                      # (1, n24)
        assert W.shape == (1, n24)
        offs, lens = segment_plan(n24, S, STRIDE)
        out.append([model.encode_codes(W[:, o:o + n].contiguous()) for o, n in zip(offs, lens)])
    return out


@pytest.fixture(scope="module")
def deep(model):
    from wavtokenizer_amd import synth
    from wavtokenizer_amd.segmented import segment_plan
    wav = torch.from_numpy(synth.make_clips(1, DEEP[0], seed=77)).cuda()
    offs, lens = segment_plan(DEEP[0], S, DEEP[1])
    assert lens == [4800] * 5 + [4500, 3000, 1500]
    return wav[0], [model.encode_codes(wav[:, o:o + n].contiguous()) for o, n in zip(offs, lens)]


def _assert_codes(sc, want, n24, stride, what):
    from wavtokenizer_amd import ARCH_HOP600
    assert (sc.length, sc.segment_length, sc.stride) == (n24, S, stride) and sc.n_segments == len(want)
    assert sc.codes.dtype == torch.int64 and sc.codes.is_cuda and sc.offsets.device.type == "cpu"
    sc.validate(ARCH_HOP600)
    for i, (g, w) in enumerate(zip(sc.segments(), want)):
        assert g.shape == w.shape == (1, 1, w.shape[-1]), (what, i, g.shape, w.shape)
        assert torch.equal(g, w), (what, i, int((g != w).sum()))


def _encode(model, sources, order):
    clips = [sources[j][0] for j in order]
    rates = [RECORDINGS[j][1] for j in order]
    return model.encode_codes_segmented_many(clips, S, STRIDE, sample_rates=rates, channels_last=True, bandwidth_id=_bw())


@pytest.fixture(scope="module")
def coded(model, sources, want_codes):
    """The recordings tokenised in one call (what the synthesis tests start from)."""
    return _encode(model, sources, range(len(RECORDINGS)))


def test_every_segment_has_the_codes_of_its_own_encode_codes_call(model, sources, want_codes, coded):
    assert [sc.n_segments for sc in coded] == [2, 2, 1, 3, 2, 1, 2, 71]
    assert [int(sc.offsets[-1]) for sc in coded] == [8 + 2, 8 + 3, 5, 8 + 8 + 2, 8 + 6, 1, 7 + 1, 560 + 2]
    base = coded[0].codes.untyped_storage().data_ptr()
    assert all(sc.codes.untyped_storage().data_ptr() == base for sc in coded)                # views of one flat tensor
    for j, sc in enumerate(coded):
        _assert_codes(sc, want_codes[j], RECORDINGS[j][0], STRIDE, ("many", j))
    _no_status(model)


def test_order_and_company_change_no_code(model, sources, want_codes):
    n = len(RECORDINGS)
    back = _encode(model, sources, range(n - 1, -1, -1))
    for j, sc in zip(range(n - 1, -1, -1), back):
        _assert_codes(sc, want_codes[j], RECORDINGS[j][0], STRIDE, ("reversed", j))
    for j in range(n):
        alone = model.encode_codes_segmented(sources[j][0], S, STRIDE, sample_rate=RECORDINGS[j][1], channels_last=True, bandwidth_id=_bw())
        _assert_codes(alone, want_codes[j], RECORDINGS[j][0], STRIDE, ("alone", j))
    _no_status(model)


def test_four_deep_at_a_short_stride(model, deep):
    wav, want = deep
    sc = model.encode_codes_segmented(wav, S, DEEP[1])                                       # (the codec rate, no bandwidth id)
    _assert_codes(sc, want, DEEP[0], DEEP[1], "deep")
    _no_status(model)


# ------------------------------------------------------------------------------------------------ synthesis
_X = {}


def _composition(model, mode, segs, rate, fmt, limit=LIMIT):
    """Item by item what the call replaces; the cross-faded 24 kHz rows are computed once per GEMM mode and shared."""
    from wavtokenizer_amd import audio
    from wavtokenizer_amd.segmented import segment_plan
    if mode not in _X:
        rows = []
        for sc in segs:
            _offs, lens = segment_plan(sc.length, sc.segment_length, sc.stride)
            dec = [model.decode_codes(c, bandwidth_id=_bw())[..., :n] for c, n in zip(sc.segments(), lens)]
            rows.append(audio.linear_overlap_add(dec, sc.stride)[..., :sc.length])           # (1, length)
        _X[mode] = rows
    out = []
    for X in _X[mode]:
        r = audio.convert_audio(X[:, None], 24000, rate, 1)[0]                               # (1, n_out)
        if fmt["dtype"] == torch.int16:
            r = audio.to_pcm16(r, limit=limit)
        r = r.expand(fmt["channels"], -1)
        out.append(r.t().contiguous() if fmt["channels_last"] else r.contiguous())
    return out


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape)
        assert torch.equal(g, w), (what, i, int((g != w).sum()))


@pytest.fixture(scope="module")
def segs(model, coded, deep):
    """All nine recordings of one synthesis call: the eight at stride 3600 and the four-deep one, rebuilt by hand from its codes."""
    from wavtokenizer_amd.segmented import SegmentedCodes
    return list(coded) + [SegmentedCodes.from_segments(deep[1], DEEP[0], S, DEEP[1])]


@pytest.mark.parametrize("rate", [24000, 44100])
@pytest.mark.parametrize("fmt", FORMATS, ids=["i16-stereo-interleaved", "f32-mono-planar"])
def test_synthesis_is_the_bits_of_the_composition(model, segs, fmt, rate):
    want = _composition(model, "f16x3", segs, rate, fmt)
    got = model.decode_pcm_segmented_many(segs, sample_rates=rate, limit=LIMIT, bandwidth_id=_bw(), **fmt)
    for g, sc in zip(got, segs):
        n = -(-rate * sc.length // 24000)
        assert tuple(g.shape) == ((n, 2) if fmt["channels_last"] else (1, n))
    _assert_same(got, want, "many")
    if fmt["dtype"] == torch.int16:
        top = int(LIMIT * 32768 + 0.5)
        assert max(int(g.max()) for g in got) == top and min(int(g.min()) for g in got) == -top      # the clamp is hit
        assert all(torch.equal(g[:, 0], g[:, 1]) for g in got)
    assert got[0].untyped_storage().data_ptr() == got[-1].untyped_storage().data_ptr()               # views of one flat tensor
    _no_status(model)


def test_order_company_rates_and_forms_of_the_result(model, segs):
    fmt = FORMATS[0]
    want = {rate: _composition(model, "f16x3", segs, rate, fmt) for rate in (24000, 44100)}
    rates = [(24000, 44100)[j % 2] for j in range(len(segs))]
    mixed = [want[r][j] for j, r in enumerate(rates)]
    back = model.decode_pcm_segmented_many(segs[::-1], sample_rates=rates[::-1], limit=LIMIT, bandwidth_id=_bw(), **fmt)
    _assert_same(back[::-1], mixed, "reversed")
    for j in (1, 5, 6, 8):
        alone = model.decode_pcm_segmented(segs[j], sample_rate=rates[j], limit=LIMIT, bandwidth_id=_bw(), **fmt)
        _assert_same([alone], [mixed[j]], ("alone", j))
    flat, offs = model.decode_pcm_segmented_many(segs, sample_rates=rates, limit=LIMIT, packed=True, bandwidth_id=_bw(), **fmt)
    assert offs.device.type == "cpu" and offs.tolist() == [2 * sum(w.shape[0] for w in mixed[:i]) for i in range(len(segs) + 1)]
    assert flat.is_cuda and torch.equal(flat, torch.cat([w.reshape(-1) for w in mixed]))
    # device="cpu": the same result in pinned host memory, no wait needed behind the call
    for f in FORMATS:
        w = _composition(model, "f16x3", segs, 44100, f)
        host, offs = model.decode_pcm_segmented_many(segs, sample_rates=44100, limit=LIMIT, packed=True, device="cpu", bandwidth_id=_bw(), **f)
        assert host.device.type == "cpu" and host.is_pinned() and host.dtype == f["dtype"]
        assert torch.equal(host, torch.cat([x.reshape(-1) for x in w]).cpu())
        got = model.decode_pcm_segmented_many(segs, sample_rates=44100, limit=LIMIT, device="cpu", bandwidth_id=_bw(), **f)
        _assert_same(got, [x.cpu() for x in w], "host")
    _no_status(model)


def test_f16_mode_gives_the_compositions_bits_under_that_mode(model, segs):
    try:
        model.set_gemm_precision("f16")
        half = [_composition(model, "f16", segs, 44100, fmt) for fmt in FORMATS]
        for fmt, w in zip(FORMATS, half):
            _assert_same(model.decode_pcm_segmented_many(segs, sample_rates=44100, limit=LIMIT, bandwidth_id=_bw(), **fmt), w, "f16")
    finally:
        model.set_gemm_precision("f16x3")
    full = _composition(model, "f16x3", segs, 44100, FORMATS[1])
    assert not all(torch.equal(a, b) for a, b in zip(half[1], full))                        # (the mode does change the waveform)
    _no_status(model)


def test_round_trip_against_the_oracle():
    from oracle import audio_ref
    from oracle.cpu_ref import OracleWavTokenizer
    from tests import parity_log
    from tests.util import WAV_REL_TOL, rel_l2, synth_state_dict
    from wavtokenizer_amd import NAMED_ARCHS, synth
    m = _cached("golden")
    orc = OracleWavTokenizer(NAMED_ARCHS["hop600"], synth_state_dict("hop600"))
    wav = torch.from_numpy(synth.make_clips(2, 48000, seed=9))
    for seg_len, stride in ((24000, 18000), (17777, 11111)):
        coded = m.encode_codes_segmented_many(list(wav.cuda()), seg_len, stride)
        got = torch.cat(m.decode_pcm_segmented_many(coded, dtype=torch.float32, bandwidth_id=_bw()))
        want = audio_ref.segmented_round_trip(orc, wav, seg_len, stride)
        assert got.shape == wav.shape == want.shape
        err = rel_l2(got.cpu().numpy(), want)
        parity_log.record(f"segmented_codes_round_trip[{seg_len},{stride}]", wav_rel_l2=err)
        print(f"segmented round trip ({seg_len}, {stride}): rel_l2 {err:.3e}")
        assert err < WAV_REL_TOL, (seg_len, stride, err)
    _no_status(m)


def test_uniform_batches_share_the_single_calls_plans_and_recordings():
    """What the one staging layout per plan kind protects: a uniform batch of full segments runs on encode_codes' (decode_codes')
    own plan and REPLAYS its recording, which it can only while both hand _call the same staging buffers.  Three full segments and a
    tail; B = 3 is within the graph limit."""
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, _capi, synth
    arch = NAMED_ARCHS["hop600"]
    m = WavTokenizer.from_arch(arch)                         # a model of its own: every plan it holds was made here
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, seed=321).items()}, strict=False)
    m = m.eval().to("cuda")
    seg, stride = 4800, 4200
    rec = torch.from_numpy(synth.make_clips(1, 3 * stride + 2000, seed=5)[0]).cuda()         # segments at 0, 4200, 8400 and a tail of 2000
    replays = _capi.lib.wt_plan_graph_replays

    def the_plan(kind, length):
        keys = [k for k in m._engine.plans if k[0] == kind and k[1] == 3 and k[2] == length]
        assert len(keys) == 1 and not keys[0][3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH and keys[0][3] & _capi.WT_PLAN_FLAG_GRAPH, keys
        return m._engine.plans[keys[0]][0]

    batch = torch.stack([rec[o:o + seg] for o in (0, stride, 2 * stride)])
    for _ in range(2):
        codes = m.encode_codes(batch)
    before = replays(the_plan(_capi.WT_PLAN_ENCODE, seg))
    coded = m.encode_codes_segmented(rec, seg, stride)
    assert coded.n_segments == 4 and torch.equal(torch.stack(coded.segments()[:3]).view(1, 3, 8), codes)
    assert replays(the_plan(_capi.WT_PLAN_ENCODE, seg)) == before + 1

    for _ in range(2):
        m.decode_codes(codes, bandwidth_id=_bw())
    before = replays(the_plan(_capi.WT_PLAN_DECODE_CODES, 8))
    pcm = m.decode_pcm_segmented(coded, bandwidth_id=_bw())
    assert pcm.shape == (1, rec.shape[0])
    assert replays(the_plan(_capi.WT_PLAN_DECODE_CODES, 8)) == before + 1
    _no_status(m)
