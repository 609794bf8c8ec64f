"""The R 128 meter and the true-peak ceiling through the public interface, on the GPU with the synthetic hop-600 model:
audio.true_peak(_many), loudness_range(_many) and r128_many against the C ABI (bit for bit), the two delta metrics,
audio.normalize(mode="lufs", max_true_peak_db=...) on a quiet clip with a click (the ceiling binds), on an ordinary clip (it does
not: the bits of the call without it) and on a clip without a loudness, encode_codes_many(max_true_peak_db=...) against
encode_infer on audio.normalize of each clip, and the segmented call.

The ceiling's slack: a normalised clip's true peak may reach 10^(c / 20) * (1 + 64 * 2^-24).  d_P = fp32(TP / 10^(c / 20)) and
every quotient x / d are rounded once (2^-24 relative each), and the measured true peak, before and after, is an fp32 dot
product of 12 terms with sum |h| < 1.87, off by at most 13 * 2^-24 * 1.87 of the largest sample (< 25 * 2^-24 of the true peak,
which is at least the sample peak), twice: 2 + 2 * 25 < 64."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from tests import loudness_ref as R
from tests import r128_ref as Q

pytestmark = pytest.mark.gpu

CEILING = -1.0
LIMIT = 10.0 ** (CEILING / 20.0) * (1.0 + 64.0 * 2.0 ** -24)
S, STRIDE, LENGTH = 12000, 9600, 26400                       # three segments: 12000, 12000 and one of 7200, under 400 ms
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


def _clicked(n: int, seed: int, where: int) -> torch.Tensor:
    """A quiet clip (noise of 0.003) with one click of 0.5: on the GPU."""
    x = R.make_clip(n, seed=seed, amplitude=0.003)
    x[where] = 0.5
    return torch.from_numpy(x).cuda()


def _ordinary(n: int, seed: int) -> torch.Tensor:
    from wavtokenizer_amd import synth
    return torch.from_numpy(synth.make_clips(1, n, seed=seed, sample_rate=24000)[0]).cuda()


def _d_P(x: torch.Tensor, fs: int = 24000) -> float:
    tp = Q.measure_true_peak([x], fs)[0, 0]
    return float(np.float32(np.float64(tp) / 10.0 ** (CEILING / 20.0)))


def test_measuring_calls_agree_with_the_c_abi():
    from wavtokenizer_amd import audio
    a = torch.from_numpy(Q.make_stepped(100000, 24000, 9501, (-40.0, -30.0, -20.0, -14.0), 100000 / 24000 / 4 + 1e-3)).cuda()   # one pass up
    b = torch.from_numpy(np.stack([Q.make_stepped(60000, 16000, 9502, (-18.0, -28.0), 0.7), Q.make_stepped(60000, 16000, 9503, (-25.0,), 1.0)])).cuda()
    c = a[:50000]                                                            # under 3 s
    clips, rates = [a, b, c], [24000, 16000, 24000]
    lin24, lin16 = Q.measure_true_peak([a, c], 24000), Q.measure_true_peak([b], 16000)
    want = 20.0 * torch.log10(torch.from_numpy(np.stack([lin24[0], lin16[0], lin24[1]])).cuda())
    got = audio.true_peak_many(clips, rates)
    assert got.shape == (3, 2) and got.dtype == torch.float32 and got.is_cuda and _bits(got) == _bits(want)
    assert bool((got[:, 0] >= got[:, 1]).all())
    assert _bits(audio.true_peak(b, 16000)) == _bits(got[1]) and _bits(audio.true_peak(a)) == _bits(got[0])
    assert audio.true_peak(torch.zeros(100, device="cuda")).tolist() == [-math.inf, -math.inf]

    r24, m24, s24 = Q.measure_range([a, c], 24000)
    r16, m16, s16 = Q.measure_range([b], 16000)
    out, mom, sht = audio.loudness_range_many(clips, rates, series=True)
    assert out.shape == (3, 9) and out.dtype == torch.float32 and out.is_cuda
    assert _bits(out) == np.stack([r24[0], r16[0], r24[1]]).tobytes()
    for got_series, want_series in ((mom, [m24[0], m16[0], m24[1]]), (sht, [s24[0], s16[0], s24[1]])):
        assert [_bits(g) for g in got_series] == [w.tobytes() for w in want_series]
    assert [t.shape[0] for t in sht] == [Q.short_term_blocks(100000, 24000), Q.short_term_blocks(60000, 16000), 0]
    assert _bits(audio.loudness_range_many(clips, rates)) == _bits(out)
    one, m1, s1 = audio.loudness_range(b, 16000, series=True)
    assert _bits(one) == _bits(out[1]) and _bits(m1) == _bits(mom[1]) and _bits(s1) == _bits(sht[1]) and _bits(audio.loudness_range(a)) == _bits(out[0])
    assert _bits(out[:, :3]) == _bits(audio.loudness_many(clips, rates))
    assert float(out[0, 3]) > 3.0 and float(out[0, 6]) > 0 and math.isnan(float(out[2, 3])) and float(out[2, 8]) == -math.inf

    rec = audio.r128_many(clips, rates)
    assert [sorted(r) for r in rec] == [sorted(["integrated", "range", "range_low", "range_high", "true_peak", "sample_peak", "max_momentary",
                                                "max_short_term"])] * 3
    for j, r in enumerate(rec):
        assert r["integrated"] == float(out[j, 0]) and r["true_peak"] == float(got[j, 0]) and r["sample_peak"] == float(got[j, 1])
        assert r["max_momentary"] == float(out[j, 7]) and r["max_short_term"] == float(out[j, 8])
        assert (math.isnan(r["range"]) and j == 2) or r["range"] == float(out[j, 3])


def test_delta_metrics():
    from wavtokenizer_amd import audio, metrics
    x = torch.from_numpy(Q.make_stepped(100000, 24000, 9511, (-20.0, -30.0, -24.0), 1.0)).cuda()
    assert float(metrics.true_peak_delta(x, x)) == 0.0 and float(metrics.loudness_range_delta(x, x)) == 0.0
    half = metrics.true_peak_delta(x * 0.5, x)                                # (halving is exact in every product and sum)
    assert half.shape == () and abs(float(half) - 20.0 * math.log10(0.5)) <= 1e-5
    lr = metrics.loudness_range_delta_many([x * 0.5, x[:50000], x], [x, x, x[:50000]])
    assert lr.shape == (3,) and abs(float(lr[0])) <= 1e-5 and math.isnan(float(lr[1])) and math.isnan(float(lr[2]))
    tp = metrics.true_peak_delta_many([x * 0.5, torch.zeros_like(x)], [x, x], sample_rate=[24000, 24000])
    assert _bits(tp[0]) == _bits(half) and math.isnan(float(tp[1]))
    want = audio.true_peak(x * 0.5)[0] - audio.true_peak(x)[0]
    assert _bits(half) == _bits(want)


def test_normalize_under_a_true_peak_ceiling():
    from wavtokenizer_amd import audio
    quiet, plain, short = _clicked(24000, 9521, 5000), _ordinary(24000, 9522), _clicked(5000, 9523, 100) * 4.0
    # a quiet clip with one click: the loudness target alone would push the click far over full scale; the ceiling binds
    free, s_free = audio.normalize(quiet, mode="lufs")
    assert float(free.abs().max()) > 2.0
    y, s = audio.normalize(quiet, mode="lufs", max_true_peak_db=CEILING)
    d_P = _d_P(quiet)
    assert float(s) == d_P and d_P > float(s_free), (float(s), d_P, float(s_free))
    assert torch.equal(y, quiet / s)                                         # one IEEE division per sample
    after = float(Q.measure_true_peak([y], 24000)[0, 0])
    print(f"ceiling {CEILING} dBTP = {10.0 ** (CEILING / 20.0):.7f}: the clip reads {after:.7f} ({Q.db(after):.4f} dBTP), allowed {LIMIT:.7f}")
    assert after <= LIMIT, (after, LIMIT)
    assert after >= 10.0 ** (CEILING / 20.0) * (1.0 - 64.0 * 2.0 ** -24)     # (and it is used up)
    # an ordinary clip: the ceiling does not bind, the bits of the call without it
    want, s_want = audio.normalize(plain, mode="lufs", target_lufs=-30.0)
    got, s_got = audio.normalize(plain, mode="lufs", target_lufs=-30.0, max_true_peak_db=CEILING)
    assert _d_P(plain) <= float(s_want) and float(s_want) != 1.0
    assert _bits(got) == _bits(want) and _bits(s_got) == _bits(s_want)
    # a clip without a loudness (under 400 ms), however large its peak: untouched, scale 1
    assert float(short.abs().max()) == 2.0
    z, s_z = audio.normalize(short, mode="lufs", max_true_peak_db=CEILING)
    assert _bits(z) == _bits(short) and float(s_z) == 1.0
    # rows of one call are independent: (B, T) gives each row the result it has alone
    both, s_both = audio.normalize(torch.stack([quiet, plain]), mode="lufs", target_lufs=-30.0, max_true_peak_db=CEILING)
    q30, sq30 = audio.normalize(quiet, mode="lufs", target_lufs=-30.0, max_true_peak_db=CEILING)
    assert _bits(both[0]) == _bits(q30) and _bits(both[1]) == _bits(got) and _bits(s_both[0]) == _bits(sq30) and _bits(s_both[1]) == _bits(s_got)
    # the C ABI refuses nothing here and writes nothing behind its workspace or the scales
    rows = torch.stack([quiet, plain]).clone()
    sc = Q.normalize_rows_lufs_tp(rows, [24000, 24000], 24000, -30.0, CEILING)
    assert _bits(rows) == _bits(both) and _bits(sc) == _bits(s_both)


def test_encode_codes_many_hands_each_clip_the_ceiling_of_audio_normalize():
    from wavtokenizer_amd import audio
    m = _model()
    clips = [_clicked(24000, 9531, 7000), _ordinary(36000, 9532)]           # 1 s (the ceiling binds) and 1.5 s (it does not)
    kw = dict(normalize="lufs", target_lufs=-26.0, max_true_peak_db=CEILING)
    got, scales = m.encode_codes_many(clips, return_scales=True, **kw)
    free, free_scales = m.encode_codes_many(clips, return_scales=True, normalize="lufs", target_lufs=-26.0)
    assert scales.shape == (2,) and scales.dtype == torch.float32 and scales.is_cuda
    for j, x in enumerate(clips):
        W = audio.convert_audio(x[None, None], 24000, 24000, 1)[0]
        y, s = audio.normalize(W, mode="lufs", target_lufs=-26.0, max_true_peak_db=CEILING)
        want = m.encode_infer(y, bandwidth_id=_bw())[1]
        assert torch.equal(got[j], want), (j, int((got[j] != want).sum()))
        assert _bits(scales[j]) == _bits(s[0]), j
        one, s1 = m.encode_codes(W, return_scales=True, **kw)                # the one-batch call, too
        assert torch.equal(one, want) and _bits(s1) == _bits(s)
    assert float(scales[0]) == _d_P(clips[0]) and float(scales[0]) > float(free_scales[0])
    assert _bits(scales[1]) == _bits(free_scales[1]) and torch.equal(got[1], free[1])
    m.check_status()


def test_the_segmented_call_hands_the_ceiling_through():
    from wavtokenizer_amd import audio
    from wavtokenizer_amd.segmented import segment_plan
    m = _model()
    x = _clicked(LENGTH, 9541, 3000)                                         # the click lies in the first segment alone
    offs, lens = segment_plan(LENGTH, S, STRIDE)
    assert lens == [12000, 12000, 7200]
    kw = dict(normalize="lufs", target_lufs=-26.0)
    sc = m.encode_codes_segmented(x, S, STRIDE, max_true_peak_db=CEILING, **kw)
    free = m.encode_codes_segmented(x, S, STRIDE, **kw)
    W = x[None]
    for i, (o, n) in enumerate(zip(offs, lens)):
        y, s = audio.normalize(W[:, o:o + n], mode="lufs", target_lufs=-26.0, max_true_peak_db=CEILING)
        assert torch.equal(sc.segments()[i], m.encode_codes(y)), i
        assert _bits(sc.scales[i]) == _bits(s[0]), i
    assert float(sc.scales[0]) == _d_P(x[:S]) and float(sc.scales[0]) > float(free.scales[0])
    assert _bits(sc.scales[1:]) == _bits(free.scales[1:]) and float(sc.scales[2]) == 1.0
    many = m.encode_codes_segmented_many([x, x[:S]], S, STRIDE, max_true_peak_db=CEILING, **kw)
    assert torch.equal(many[0].codes, sc.codes) and _bits(many[0].scales) == _bits(sc.scales)
    m.check_status()
