"""normalize="lufs" and the loudness calls through the public interface, on the GPU with the synthetic hop-600 model:
encode_codes_many(normalize="lufs") against encode_infer on audio.normalize of each converted clip (bit for bit), the scales
against audio.normalize's, the loudness of a normalised clip against the target, the segmented round trip with a last segment too
short to have a loudness, decode_pcm(scales=...) and metrics.loudness_delta."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from tests import loudness_ref as R

pytestmark = pytest.mark.gpu

# (samples, rate, form): 14000, 13500, 13062 and 12000 samples at the codec rate, each at least 0.5 s
CLIPS = [(14000, 24000, "f32-mono-gpu"), (9000, 16000, "f32-mono-cpu"), (24000, 44100, "i16-stereo-cpu"), (24000, 48000, "i16-mono-gpu")]
S, STRIDE, LENGTH = 12000, 9600, 26400                       # three segments: 12000, 12000 and one of 7200, under 400 ms
TARGET = -23.0
_MODELS = {}


def _model():
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer, synth
    if 1 not in _MODELS:
        arch = dataclasses.replace(ARCH_HOP600, num_quantizers=1)
        sd = synth.make_state_dict(arch, seed=321)
        m = WavTokenizer.from_arch(arch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        _MODELS[1] = m.eval().to("cuda")
    return _MODELS[1]


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
        x = synth.make_clips(2, n, seed=180 + j, sample_rate=rate)
        if form.startswith("i16"):
            q = torch.from_numpy(np.rint(x * 32767.0).astype(np.int16))                       # planar (2, n)
            q = q if "stereo" in form else q[0]
            clip, planar = (q.cuda() if form.endswith("gpu") else q), (q.float() / 32768.0).cuda().view(-1, n)
        else:
            t = torch.from_numpy(x[0])
            clip, planar = (t.cuda() if form.endswith("gpu") else t), t.cuda()[None]
        out.append((clip, audio.convert_audio(planar[None], rate, 24000, 1)[0]))
    assert [w.shape[-1] for _c, w in out] == [14000, 13500, 13062, 12000]
    return out


def test_encode_codes_many_normalises_each_clip_like_audio_normalize(sources):
    from wavtokenizer_amd import audio
    m = _model()
    kw = dict(normalize="lufs", target_lufs=-23)
    rates = [r for _n, r, _f in CLIPS]
    got, scales = m.encode_codes_many([c for c, _w in sources], sample_rates=rates, return_scales=True, **kw)
    plain = m.encode_codes_many([c for c, _w in sources], sample_rates=rates)
    assert scales.shape == (len(CLIPS),) and scales.dtype == torch.float32 and scales.is_cuda
    differs = 0
    for j, (_clip, W) in enumerate(sources):
        y, s = audio.normalize(W, mode="lufs", target_lufs=-23)
        want = m.encode_infer(y, bandwidth_id=_bw())[1]
        assert torch.equal(got[j], want), (j, int((got[j] != want).sum()))
        assert _bits(scales[j]) == _bits(s[0]), j
        assert float(s[0]) != 1.0 and math.isfinite(float(s[0]))
        differs += int((got[j] != plain[j]).sum())
        one, s1 = m.encode_codes(W, return_scales=True, **kw)                               # the one-batch call, too
        assert torch.equal(one, want) and _bits(s1) == _bits(s)
    assert differs > 0                                         # (the normalisation reaches the codes)
    default = m.encode_codes_many([c for c, _w in sources], sample_rates=rates, normalize="lufs")      # the default target is -23
    assert all(torch.equal(a, b) for a, b in zip(default, got))
    other = m.encode_codes_many([c for c, _w in sources], sample_rates=rates, normalize="lufs", target_lufs=-16.0, return_scales=True)[1]
    ratio = (scales.double() / other.double()).cpu().numpy()                                # 7 dB apart: 10^(7 / 20) within the roundings
    assert np.abs(ratio / 10.0 ** (7.0 / 20.0) - 1.0).max() <= 2.0 ** -22
    m.check_status()


def test_a_normalised_clip_reads_the_target(sources):
    """audio.loudness of audio.normalize's output: within the measurement's bound on this clip (tests/loudness_ref.py: the fp32
    lfilter evaluation's error, at least two ulps) plus one ulp of the division: the rounding of the divisor and of the quotients,
    2^-24 relative each, 2 * 20 log10(1 + 2^-24) LU."""
    from wavtokenizer_amd import audio
    for j, (_clip, W) in enumerate(sources):
        x = W[0].cpu().numpy()
        ref, f32 = R.loudness(x, 24000), R.loudness(x, 24000, np.float32)
        assert R.gate_margin(x, 24000) >= 0.01, j
        first = audio.loudness(W[0])
        assert first.shape == (3,) and abs(float(first[0]) - ref[0]) <= R.bound(ref[0], f32[0]) and float(first[2]) == ref[2], j
        y, s = audio.normalize(W, mode="lufs", target_lufs=TARGET)
        assert float(s[0]) == float(np.float32(10.0 ** ((float(first[0]) - TARGET) / 20.0))), j      # d from the fp32 L, in double
        assert torch.equal(y.cpu(), W.cpu() / s[0].cpu()), j                                 # one IEEE division per sample
        again = audio.loudness(y[0])
        tol = R.bound(ref[0], f32[0]) + 2 * 20.0 * math.log10(1.0 + 2.0 ** -24)
        print(f"normalised clip {j}: reads {float(again[0]):.7f}, |error| {abs(float(again[0]) - TARGET):.3e}, allowed {tol:.3e}")
        assert abs(float(again[0]) - TARGET) <= tol, (j, float(again[0]), tol)
    # many clips, two rates, stereo, momentary values: rows in input order, whatever the grouping by rate
    a, b = sources[0][1][0], sources[3][1][0]
    st = torch.stack([b, b.flip(0)])
    out, blocks = audio.loudness_many([a, st, b, a[:9000]], [24000, 16000, 24000, 24000], momentary=True)
    assert out.shape == (4, 3) and [t.shape[0] for t in blocks] == [R.blocks(14000, 24000), R.blocks(12000, 16000), R.blocks(12000, 24000), 0]
    assert [t.shape[0] for t in blocks] == [2, 4, 2, 0]
    assert _bits(out[0]) == _bits(audio.loudness(a)) and _bits(out[2]) == _bits(audio.loudness(b, 24000))
    assert _bits(out[1]) == _bits(audio.loudness(st, 16000)) and out[3].tolist() == [-math.inf, -math.inf, 0.0]
    assert math.isfinite(float(out[1][0]))
    want, want32 = R.loudness(st.cpu().numpy(), 16000), R.loudness(st.cpu().numpy(), 16000, np.float32)
    assert abs(float(out[1][0]) - want[0]) <= R.bound(want[0], want32[0])
    for g, w, w32 in zip(blocks[1].cpu().numpy(), want[3], want32[3]):
        assert abs(float(g) - w) <= R.bound(w, w32)


def test_segmented_round_trip_with_a_last_segment_under_400_ms():
    from wavtokenizer_amd import audio, synth
    from wavtokenizer_amd.segmented import segment_plan
    m = _model()
    rate = 16000
    x = torch.from_numpy(synth.make_clips(1, 17600, seed=197, sample_rate=rate)).cuda()     # 17 600 at 16 kHz: 26 400 at the codec rate
    W = audio.convert_audio(x[None], rate, 24000, 1)[0]
    assert W.shape == (1, LENGTH)
    offs, lens = segment_plan(LENGTH, S, STRIDE)
    assert lens == [12000, 12000, 7200]
    sc = m.encode_codes_segmented(x[0], S, STRIDE, sample_rate=rate, normalize="lufs", target_lufs=TARGET)
    assert sc.scales.shape == (3,) and sc.scales.dtype == torch.float32 and sc.scales.is_cuda
    assert float(sc.scales[2]) == 1.0 and float(sc.scales[0]) != 1.0 and float(sc.scales[1]) != 1.0
    frames = []
    for i, (o, n) in enumerate(zip(offs, lens)):
        y, s = audio.normalize(W[:, o:o + n], mode="lufs", target_lufs=TARGET)
        if i == 2:
            assert torch.equal(y, W[:, o:o + n])               # under 400 ms: as it is, bit for bit
        want = m.encode_codes(y)
        assert torch.equal(sc.segments()[i], want), i
        assert _bits(sc.scales[i]) == _bits(s[0]), i
        frames.append(m.decode_codes(want[0], bandwidth_id=_bw())[..., :n] * s[0])          # _decode_frame's out * scale
    X = audio.linear_overlap_add(frames, STRIDE)[..., :LENGTH]
    want = audio.convert_audio(X[:, None], 24000, rate, 1)[0]
    got = m.decode_pcm_segmented(sc, sample_rate=rate, dtype=torch.float32, channels=1, bandwidth_id=_bw())
    assert got.shape == want.shape and torch.equal(got, want), int((got != want).sum())
    many = m.encode_codes_segmented_many([x[0], x[0, :12000]], S, STRIDE, sample_rates=rate, normalize="lufs")
    assert torch.equal(many[0].codes, sc.codes) and _bits(many[0].scales) == _bits(sc.scales)
    m.check_status()


def test_decode_pcm_multiplies_the_scales_back_in(sources):
    from wavtokenizer_amd import audio
    m = _model()
    W = [w for _c, w in sources]
    codes, scales = m.encode_codes_many([w[0] for w in W], normalize="lufs", target_lufs=TARGET, return_scales=True)
    rate = 16000
    got = m.decode_pcm_many([c[0] for c in codes], sample_rates=rate, dtype=torch.float32, bandwidth_id=_bw(), scales=scales)
    for j, c in enumerate(codes):
        r = audio.convert_audio((m.decode_codes(c[0], bandwidth_id=_bw()) * scales[j])[:, None], 24000, rate, 1)[0]
        assert torch.equal(got[j], r), j
        one = m.decode_pcm(c[0], sample_rate=rate, dtype=torch.float32, bandwidth_id=_bw(), scales=scales[j:j + 1])
        assert torch.equal(one[0], r), j
    m.check_status()


def test_loudness_delta(sources):
    from wavtokenizer_amd import metrics
    x = sources[0][1][0]
    ref, f32 = R.loudness(x.cpu().numpy(), 24000), R.loudness(x.cpu().numpy(), 24000, np.float32)
    same = metrics.loudness_delta(x, x)
    assert same.shape == () and float(same) == 0.0
    half = metrics.loudness_delta(x * 0.5, x)                   # (the halves are exact: every block moves by 20 log10 0.5 = -6.0206)
    assert abs(float(half) - 20.0 * math.log10(0.5)) <= R.bound(ref[0], f32[0]), float(half)
    st = torch.stack([x, x])
    d = metrics.loudness_delta_many([x * 0.5, st, x[:9000], x], [x, x, x, torch.zeros_like(x)], sample_rate=[24000, 24000, 24000, 24000])
    assert d.shape == (4,) and _bits(d[0]) == _bits(half)
    assert abs(float(d[1]) - 10.0 * math.log10(2.0)) <= 4 * R.ulp32(ref[0])     # the same signal in two channels: twice the energy; two fp32 readings
    assert math.isnan(float(d[2])) and math.isnan(float(d[3]))  # under 400 ms; against silence
