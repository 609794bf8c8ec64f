"""Per-clip level control through the public calls, on the GPU with the synthetic hop-600 model: encode_codes_many(normalize=...)
against encode_infer on audio.normalize of each converted clip, return_scales against audio.normalize's scale, the invariance of
peak mode under a power-of-two gain, the segmented round trip with Encodec's per-segment scales against the per-segment
composition, and decode_pcm(_many)(rescale=True / scales=...) against the one-clip compositions; everything bit for bit."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (samples, rate, form): resampled lengths 6000, 4097, 1633, 1024, 3000
CLIPS = [(6000, 24000, "f32-mono-gpu"), (2731, 16000, "f32-mono-cpu"), (3000, 44100, "i16-stereo-cpu"), (1024, 24000, "f32-mono-gpu"),
         (2000, 16000, "f32-mono-gpu")]
S, STRIDE, LENGTH = 4800, 3600, 12000                         # four segments: 4800, 4800, 4800 and a short one of 1200
LIMIT = 0.25
_MODELS = {}


def _model(n_q=1):
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer, synth
    if n_q not in _MODELS:
        arch = dataclasses.replace(ARCH_HOP600, num_quantizers=n_q)
        sd = synth.make_state_dict(arch, seed=321)
        m = WavTokenizer.from_arch(arch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        _MODELS[n_q] = m.eval().to("cuda")
    return _MODELS[n_q]


def _bw():
    return torch.tensor([0])


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def sources():
    """Per clip (the clip as the caller holds it, the same clip at the codec rate: (1, n24) fp32 on the GPU); computed once."""
    from wavtokenizer_amd import audio, synth
    out = []
    for j, (n, rate, form) in enumerate(CLIPS):
        x = synth.make_clips(2, n, seed=80 + j, sample_rate=rate)
        if form.startswith("i16-stereo"):
            q = torch.from_numpy(np.rint(x * 32767.0).astype(np.int16))                       # planar (2, n) on the CPU
            clip, planar = q, (q.float() / 32768.0).cuda()
        else:
            t = torch.from_numpy(x[0])
            clip, planar = (t.cuda() if form.endswith("gpu") else t), t.cuda()[None]
        out.append((clip, audio.convert_audio(planar[None], rate, 24000, 1)[0]))
    assert [w.shape[-1] for _c, w in out] == [6000, 4097, 1633, 1024, 3000]
    return out


@pytest.mark.parametrize("mode,target_db", [("peak", 0.0), ("rms", 0.0), ("peak", -3.0)])
def test_encode_codes_many_normalises_each_clip_like_audio_normalize(sources, mode, target_db):
    from wavtokenizer_amd import audio
    m = _model()
    kw = dict(normalize=mode, target_db=target_db)
    got, scales = m.encode_codes_many([c for c, _w in sources], sample_rates=[r for _n, r, _f in CLIPS], return_scales=True, **kw)
    plain = m.encode_codes_many([c for c, _w in sources], sample_rates=[r for _n, r, _f in CLIPS])
    assert scales.shape == (len(CLIPS),) and scales.dtype == torch.float32 and scales.is_cuda
    differs = 0
    for j, (_clip, W) in enumerate(sources):
        y, s = audio.normalize(W, mode, target_db)
        want = m.encode_infer(y, bandwidth_id=_bw())[1]
        assert torch.equal(got[j], want), (mode, target_db, j, int((got[j] != want).sum()))
        assert _bits(scales[j]) == _bits(s[0]), (mode, j)
        differs += int((got[j] != plain[j]).sum())
        one, s1 = m.encode_codes(W, return_scales=True, **kw)                               # the one-batch call, too
        assert torch.equal(one, want) and _bits(s1) == _bits(s)
    assert differs > 0                                         # (the normalisation reaches the codes: the clips peak near 0.4)
    flat, offsets, packed_scales = m.encode_codes_many([c for c, _w in sources], sample_rates=[r for _n, r, _f in CLIPS], packed=True,
                                                       return_scales=True, **kw)
    assert torch.equal(flat, torch.cat([g.view(-1) for g in got])) and _bits(packed_scales) == _bits(scales)
    assert offsets.tolist() == [0, 10, 17, 20, 22, 27]
    m.check_status()


def test_residual_vq_after_the_normalisation(sources):
    from wavtokenizer_amd import audio
    m = _model(3)
    got = m.encode_codes_many([c for c, _w in sources], sample_rates=[r for _n, r, _f in CLIPS], n_q=2, normalize="peak")
    for j, (_clip, W) in enumerate(sources):
        want = m.encode_codes(audio.normalize(W, "peak")[0], n_q=2)
        assert got[j].shape == want.shape == (2, 1, want.shape[-1]) and torch.equal(got[j], want), j


def test_peak_mode_does_not_see_a_power_of_two_gain():
    """Unless 1e-8 reaches the sum: both copies peak where peak + 1e-8f == peak in fp32 (half a unit of 0.25 is 1.5e-8), so x / d
    has the same bits for both, and so have the codes."""
    from wavtokenizer_amd import synth
    m = _model()
    loud = [synth.make_clips(1, n, seed=90 + j)[0] * np.float32(256.0) for j, n in enumerate((6000, 3000, 1024))]
    quiet = [x * np.float32(2.0 ** -7) for x in loud]
    for x in loud + quiet:                                                                   # asserted on the CPU first
        peak = np.abs(x).max()
        assert peak >= 0.25 and np.float32(peak) + np.float32(1e-8) == np.float32(peak)
    a, sa = m.encode_codes_many([torch.from_numpy(x) for x in loud], normalize="peak", return_scales=True)
    b, sb = m.encode_codes_many([torch.from_numpy(x) for x in quiet], normalize="peak", return_scales=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert torch.equal(sa * 2.0 ** -7, sb)
    raw = m.encode_codes_many([torch.from_numpy(x) for x in quiet])
    assert any(not torch.equal(p, q) for p, q in zip(raw, b))                               # (without it the quiet copy codes differently)


def test_segmented_round_trip_with_per_segment_scales():
    from wavtokenizer_amd import audio, synth
    from wavtokenizer_amd.segmented import SegmentedCodes, segment_plan
    m = _model()
    rate = 16000
    x = torch.from_numpy(synth.make_clips(1, 8000, seed=97, sample_rate=rate)).cuda()      # 8000 at 16 kHz: 12 000 at the codec rate
    W = audio.convert_audio(x[None], rate, 24000, 1)[0]
    assert W.shape == (1, LENGTH)
    offs, lens = segment_plan(LENGTH, S, STRIDE)
    assert lens == [4800, 4800, 4800, 1200]
    sc = m.encode_codes_segmented(x[0], S, STRIDE, sample_rate=rate, normalize="rms")
    plain = m.encode_codes_segmented(x[0], S, STRIDE, sample_rate=rate)
    assert plain.scales is None and sc.scales.shape == (4,) and sc.scales.dtype == torch.float32 and sc.scales.is_cuda
    frames, frames_plain = [], []
    for i, (o, n) in enumerate(zip(offs, lens)):
        y, s = audio.normalize(W[:, o:o + n], "rms")
        want = m.encode_codes(y)
        assert torch.equal(sc.segments()[i], want), i
        assert _bits(sc.scales[i]) == _bits(s[0]), i
        frames.append(m.decode_codes(want[0], bandwidth_id=_bw())[..., :n] * s[0])          # _decode_frame's out * scale
        frames_plain.append(m.decode_codes(want[0], bandwidth_id=_bw())[..., :n])
    for fmt in (dict(dtype=torch.int16, channels=2, channels_last=True), dict(dtype=torch.float32, channels=1)):
        for fr, seg in ((frames, sc), (frames_plain, SegmentedCodes(sc.codes, sc.offsets, LENGTH, S, STRIDE, None))):
            X = audio.linear_overlap_add(fr, STRIDE)[..., :LENGTH]
            r = audio.convert_audio(X[:, None], 24000, rate, 1)[0]
            want = audio.to_pcm16(r, limit=LIMIT) if fmt["dtype"] == torch.int16 else r
            want = want.expand(fmt["channels"], -1)
            want = want.t() if fmt.get("channels_last") else want
            got = m.decode_pcm_segmented(seg, sample_rate=rate, limit=LIMIT, bandwidth_id=_bw(), **fmt)
            assert got.shape == want.shape and torch.equal(got, want), (fmt, seg.scales is None, int((got != want).sum()))
    # rescale on the cross-faded recording
    X = audio.linear_overlap_add(frames, STRIDE)[..., :LENGTH]
    r = audio.convert_audio(X[:, None], 24000, rate, 1)[0]
    got = m.decode_pcm_segmented(sc, sample_rate=rate, limit=LIMIT, bandwidth_id=_bw(), rescale=True)
    assert torch.equal(got, audio.to_pcm16(r, rescale=True, limit=LIMIT))
    m.check_status()


@pytest.mark.parametrize("n", [1, 65])
def test_decode_pcm_many_rescaled_is_the_one_clip_composition(n):
    from tests import level_ref as R
    from wavtokenizer_amd import audio
    m = _model()
    g = torch.Generator().manual_seed(5 + n)
    rates = [16000, 24000, 44100]
    codes = [torch.randint(0, 4096, (1, 2 + (j * 5) % 7), generator=g).cuda() for j in range(n)]
    sr = [rates[j % 3] for j in range(n)]
    ch = [1 + j % 2 for j in range(n)]
    for dtype in (torch.int16, torch.float32):
        got = m.decode_pcm_many(codes, sample_rates=sr, channels=ch, dtype=dtype, limit=LIMIT, bandwidth_id=_bw(), rescale=True)
        scaled_down = 0
        for j in range(n):
            f32 = m.decode_pcm(codes[j], sample_rate=sr[j], dtype=torch.float32, bandwidth_id=_bw())[0, 0]
            want = audio.to_pcm16(f32, rescale=True, limit=LIMIT) if dtype == torch.int16 else f32 * R.rescale_factor(f32, LIMIT)
            assert got[j].shape == (ch[j], want.shape[0])
            for c in range(ch[j]):
                assert torch.equal(got[j][c], want), (n, dtype, j, c)
            scaled_down += float(f32.abs().max()) > LIMIT
            if j < 5:                                           # (the one-clip call: the first clips of the big batch are enough)
                one = m.decode_pcm(codes[j], sample_rate=sr[j], channels=ch[j], dtype=dtype, limit=LIMIT, bandwidth_id=_bw(), rescale=True)
                assert torch.equal(one[0], got[j]), (n, dtype, j)
        assert scaled_down > 0                                  # (the synthetic decoder's waveforms peak above the limit)
    m.check_status()


def test_decode_pcm_multiplies_the_scales_back_in(sources):
    from wavtokenizer_amd import audio
    m = _model()
    W = [w for _c, w in sources]
    codes, scales = m.encode_codes_many([w[0] for w in W], normalize="rms", return_scales=True)
    rate = 16000
    got = m.decode_pcm_many([c[0] for c in codes], sample_rates=rate, dtype=torch.float32, bandwidth_id=_bw(), scales=scales)
    for j, c in enumerate(codes):
        r = audio.convert_audio((m.decode_codes(c[0], bandwidth_id=_bw()) * scales[j])[:, None], 24000, rate, 1)[0]
        assert torch.equal(got[j], r), j
        one = m.decode_pcm(c[0], sample_rate=rate, dtype=torch.float32, bandwidth_id=_bw(), scales=scales[j:j + 1])
        assert torch.equal(one[0], r), j
    m.check_status()
