"""The Python surface of the pitch / periodicity metrics (wavtokenizer_amd/metrics.py) and WavTokenizer.round_trip_periodicity /
round_trip_report(periodicity=True) on the GPU: the clips of tests/test_pitch_op.py through Python give the bits of the C ABI, the
one-clip calls' bits at any position of a list, other sample rates, graph capture, and the report against the separate call."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pitch_ref as R
from tests.util import synth_state_dict

pytestmark = pytest.mark.gpu


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def test_the_test_clips_through_python_have_the_bits_of_the_c_abi_and_meet_float64():
    from wavtokenizer_amd import metrics
    c = R.cases()
    want, ok = R.run_track(c.signals, taps=False)
    got = metrics.pitch_many([_cuda(x) for x in c.signals])
    assert ok and len(got) == len(want)
    for (f0, per), w, t in zip(got, want, c.t64):
        assert f0.shape == per.shape == (t.n,) and f0.dtype == per.dtype == torch.float32
        assert np.array_equal(f0.cpu().numpy(), w[0], equal_nan=True) and np.array_equal(per.cpu().numpy(), w[1])
    refs, ests = [c.signals[i] for i, _ in c.pairs], [c.signals[j] for _, j in c.pairs]
    want, ok = R.run_pairs(refs, ests)
    m = metrics.periodicity_metrics_many([_cuda(x) for x in refs], [_cuda(x) for x in ests])
    assert ok and m.shape == (len(refs), 3) and m.dtype == torch.float32 and np.array_equal(m.cpu().numpy(), np.stack(want), equal_nan=True)
    for (i, j), g in zip(c.pairs, m.cpu().numpy()):
        ours = [SimpleNamespace(f0=got[k][0].cpu().numpy(), per=got[k][1].cpu().numpy()) for k in (i, j)]
        w64 = c.pair_want(i, j, *ours)
        assert bool((R.metric_error(g, w64) <= c.pair_bar(w64)).all()), (i, j, g, w64)


def test_many_forms_have_the_bits_of_the_one_clip_calls():
    from wavtokenizer_amd import metrics
    c = R.cases()
    xs = [_cuda(c.signals[0][:T]) for T in (5000, 1024, 1184, 7001)]
    ys = [_cuda(c.signals[2][:T]) for T in (5000, 1024, 1184, 7001)]
    tracks = metrics.pitch_many(xs)
    m = metrics.periodicity_metrics_many(xs, ys)
    for i, (x, y) in enumerate(zip(xs, ys)):
        f0, per = metrics.pitch(x)
        assert torch.equal(per, tracks[i][1]) and np.array_equal(f0.cpu().numpy(), tracks[i][0].cpu().numpy(), equal_nan=True)
        assert f0.shape == (metrics.pitch_frames(x.shape[0]),)
        one = metrics.periodicity_metrics(x, y)
        assert one.shape == (3,) and np.array_equal(one.cpu().numpy(), m[i].cpu().numpy(), equal_nan=True)
    # the keywords reach the kernels: nothing unvoiced, nothing silent; a threshold every lag meets gives the first local minimum
    f0, per = metrics.pitch(xs[0], silence_threshold=-1e30, unvoiced_threshold=-1.0)
    assert not bool(torch.isnan(f0).any()) and bool(torch.isnan(tracks[0][0]).any())
    f0_min, _ = metrics.pitch(xs[0], threshold=10.0, silence_threshold=-1e30, unvoiced_threshold=-1.0)
    assert not torch.equal(f0_min, f0)
    z = torch.zeros(3000, device="cuda")
    out = metrics.periodicity_metrics(z, z).cpu().numpy()
    assert out[0] == 0 and np.isnan(out[1]) and np.isnan(out[2]) and bool((metrics.pitch(z)[1] == 0).all())
    assert metrics.periodicity_metrics_many([], []).shape == (0, 3)
    assert bool(torch.equal(metrics.pitch(xs[0].double())[1], tracks[0][1]))                     # other floating types are cast


def test_other_sample_rates_go_through_the_package_resampler():
    from wavtokenizer_amd import audio, metrics
    c = R.cases()
    x, y = _cuda(c.signals[0][:12000]), _cuda(c.signals[2][:12000])        # read as 24 kHz audio: 8000 samples at 16 kHz
    x16, y16 = (audio.convert_audio(t.view(1, -1), 24000, 16000)[0].contiguous() for t in (x, y))
    assert x16.shape == (8000,)
    f0, per = metrics.pitch(x, 24000)
    g0, qer = metrics.pitch(x16)
    assert per.shape == (44,) and torch.equal(per, qer) and np.array_equal(f0.cpu().numpy(), g0.cpu().numpy(), equal_nan=True)
    m = metrics.periodicity_metrics_many([x, x16], [y, y16], sample_rate=[24000, 16000]).cpu().numpy()
    assert np.array_equal(m[0], m[1], equal_nan=True) and np.isfinite(m[0][0])


def test_up_to_64_pairs_are_capturable_in_a_graph():
    """Up to 64 descriptors travel in the launches' argument blocks: no copy and no host wait, so the calls can be captured."""
    from wavtokenizer_amd import metrics
    c = R.cases()
    lengths = (1024, 1500, 2047, 4100)
    xs = [_cuda(c.signals[4 * (i % 2)][31 * i:31 * i + lengths[i % 4]]) for i in range(64)]
    ys = [_cuda(c.signals[4 * (i % 2) + 1 + i % 3][31 * i:31 * i + lengths[i % 4]]) for i in range(64)]
    eager = metrics.periodicity_metrics_many(xs, ys)
    eager_track = metrics.pitch(xs[3])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.periodicity_metrics_many(xs, ys)                       # (warm-up on the capture stream)
        metrics.pitch(xs[3])
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = metrics.periodicity_metrics_many(xs, ys)
        got_track = metrics.pitch(xs[3])
    got.zero_()
    got_track[1].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), eager.cpu().numpy(), equal_nan=True) and torch.equal(got_track[1], eager_track[1])
    assert np.array_equal(got_track[0].cpu().numpy(), eager_track[0].cpu().numpy(), equal_nan=True)
    # the graph reads the inputs where they are: new contents, new result, the bits of the eager call on them
    xs[3].copy_(ys[3])
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), metrics.periodicity_metrics_many(xs, ys).cpu().numpy(), equal_nan=True)
    assert got[3, 0] == 0 and not np.array_equal(got.cpu().numpy(), eager.cpu().numpy(), equal_nan=True)


def test_round_trip_report_with_periodicity():
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer, metrics, synth
    sd = synth_state_dict("hop600")
    m = WavTokenizer.from_arch(ARCH_HOP600)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    m = m.eval().to("cuda")
    wavs = [torch.from_numpy(synth.make_clips(1, T, seed=40 + i)[0]).cuda() for i, T in enumerate((12000, 19999, 28800))]
    bw = torch.tensor([0])
    three = m.round_trip_periodicity(wavs, bandwidth_id=bw)
    assert three.shape == (3, 3) and three.dtype == torch.float32 and bool(torch.isfinite(three[:, 0]).all())
    outs = m.decode_codes_many(m.encode_codes_many(wavs, bandwidth_id=bw), bandwidth_id=bw)
    crops = [o[0, :w.shape[0]] for o, w in zip(outs, wavs)]
    assert np.array_equal(three.cpu().numpy(), metrics.periodicity_metrics_many(wavs, crops, sample_rate=24000).cpu().numpy(), equal_nan=True)
    rep = m.round_trip_report(wavs, bandwidth_id=bw, extended=True, periodicity=True)
    assert list(rep) == ["mel_distance", "stoi", "estoi", "stft_distance", "si_sdr", "snr", "periodicity_loss", "pitch_loss", "vuv_f1"]
    for k, name in enumerate(("periodicity_loss", "pitch_loss", "vuv_f1")):
        assert rep[name].shape == (3,) and np.array_equal(rep[name].cpu().numpy(), three[:, k].cpu().numpy(), equal_nan=True)
    plain = m.round_trip_report(wavs, bandwidth_id=bw)
    assert list(plain) == ["mel_distance", "stoi", "stft_distance", "si_sdr", "snr"]              # the default is as it was
    assert all(torch.equal(plain[k], rep[k]) for k in plain)
    empty = m.round_trip_report([], bandwidth_id=bw, periodicity=True)
    assert list(empty)[-3:] == ["periodicity_loss", "pitch_loss", "vuv_f1"] and all(v.shape == (0,) for v in empty.values())
    assert m.round_trip_periodicity([], bandwidth_id=bw).shape == (0, 3)
