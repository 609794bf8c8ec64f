"""The Python surface of the STFT distance, SI-SDR and SNR (wavtokenizer_amd/metrics.py) and WavTokenizer.round_trip_report on the
GPU: shapes, the bits of the one-pair calls at any position of a list and in the (B, T) forms, and the report against the separate
round trips."""
import numpy as np
import pytest
import torch

from tests import stftd_ref as S
from tests import wavedist_ref as W
from tests.util import synth_state_dict

pytestmark = pytest.mark.gpu


def _pair(i, T=3001):
    y = S.signal("noise_tone", T, seed=50 + i)
    return torch.from_numpy(S.estimate_of("noise_tone", y)).cuda(), torch.from_numpy(y).cuda()


def test_shapes_and_values():
    from wavtokenizer_amd import metrics
    x, y = _pair(0)
    d = metrics.stft_distance(x, y)
    d64, c64 = S.distance64(x.cpu().numpy(), y.cpu().numpy())
    assert d.shape == () and d.dtype == torch.float32 and abs(float(d) - d64) <= 1e-5 * d64
    d2, c = metrics.stft_distance(x, y, components=True)
    assert torch.equal(d, d2) and c.shape == (3, 2) and float((c.cpu().double() - torch.from_numpy(c64)).abs().max()) <= 1e-5
    assert float(d) == float(S.total_fp32(c.cpu().numpy()))
    m = metrics.stft_magnitude(x, 1024, 120, 600)
    assert m.shape == (513, 1 + 3001 // 120)
    assert float((m.cpu().double() - torch.from_numpy(S.magnitude64(x.cpu().numpy(), 1024, 120, 600)[0])).abs().max()) < 1e-4
    one = metrics.stft_distance(x, y, fft_sizes=(512,), hop_sizes=(50,), win_lengths=(240,), components=True)
    assert one[1].shape == (1, 2) and torch.equal(one[1][0], c[2]) and float(one[0]) == float(np.float32(c[2, 0].item()) + np.float32(c[2, 1].item()))
    s, n = metrics.si_sdr(x, y), metrics.snr(x, y)
    w = W.measures64(x.cpu().numpy(), y.cpu().numpy())
    assert s.shape == () and n.shape == () and abs(float(s) - w[0]) < 0.01 and abs(float(n) - w[1]) < 0.01
    wz = W.measures64(x.cpu().numpy() + 0.3, y.cpu().numpy() - 0.2, zero_mean=True)
    assert abs(float(metrics.si_sdr(x + 0.3, y - 0.2, zero_mean=True)) - wz[0]) < 0.01
    assert abs(float(metrics.snr(x + 0.3, y - 0.2, True)) - wz[1]) < 0.01
    z = torch.zeros(3001, device="cuda")
    assert float(metrics.stft_distance(z, z)) == 0.0 and float(metrics.si_sdr(z, z)) == 0.0 and float(metrics.snr(z, z)) == 0.0
    assert metrics.stft_distance_many([], []).shape == (0,) and metrics.si_sdr_many([], []).shape == (0,)
    assert metrics.stft_magnitude_many([]) == []


def test_many_and_batch_forms_have_the_bits_of_the_one_pair_calls():
    from wavtokenizer_amd import metrics
    pairs = [_pair(i, T) for i, T in enumerate((3001, 1025, 4100, 3001))]
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    d, c = metrics.stft_distance_many(xs, ys, components=True)
    s, n = metrics.si_sdr_many(xs, ys), metrics.snr_many(xs, ys)
    sz = metrics.si_sdr_many(xs, ys, zero_mean=True)
    mags = metrics.stft_magnitude_many(xs, 2048, 240, 1200)
    assert d.shape == (4,) and c.shape == (4, 3, 2) and s.shape == (4,) and n.shape == (4,)
    for i, (x, y) in enumerate(pairs):
        di, ci = metrics.stft_distance(x, y, components=True)
        assert torch.equal(d[i], di) and torch.equal(c[i], ci)
        assert torch.equal(s[i], metrics.si_sdr(x, y)) and torch.equal(n[i], metrics.snr(x, y))
        assert torch.equal(sz[i], metrics.si_sdr(x, y, zero_mean=True))
        assert torch.equal(mags[i], metrics.stft_magnitude(x, 2048, 240, 1200))
    X, Y = torch.stack([xs[0], xs[3]]), torch.stack([ys[0], ys[3]])
    for form in (lambda t: t, lambda t: t[:, None, :]):
        db, cb = metrics.stft_distance(form(X), form(Y), components=True)
        assert db.shape == (2,) and cb.shape == (2, 3, 2)
        assert torch.equal(db, d[[0, 3]]) and torch.equal(cb, c[[0, 3]])
        assert torch.equal(metrics.si_sdr(form(X), form(Y)), s[[0, 3]]) and torch.equal(metrics.snr(form(X), form(Y)), n[[0, 3]])
    assert torch.equal(metrics.stft_magnitude(X, 2048, 240, 1200), torch.stack([mags[0], mags[3]]))
    assert metrics.stft_magnitude(X[:, None, :], 2048, 240, 1200).shape == (2, 1, 1025, 13)


def test_round_trip_report():
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer, metrics, synth
    sd = synth_state_dict("hop600")
    m = WavTokenizer.from_arch(ARCH_HOP600)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    m = m.eval().to("cuda")
    wavs = [torch.from_numpy(synth.make_clips(1, T, seed=40 + i)[0]).cuda() for i, T in enumerate((12000, 19999, 28800))]
    bw = torch.tensor([0])
    codes = m.encode_codes_many(wavs, bandwidth_id=bw)
    outs = m.decode_codes_many(codes, bandwidth_id=bw)
    crops = [o[0, :w.shape[0]] for o, w in zip(outs, wavs)]
    rep = m.round_trip_report(wavs, bandwidth_id=bw, extended=True)
    assert list(rep) == ["mel_distance", "stoi", "estoi", "stft_distance", "si_sdr", "snr"]
    for v in rep.values():
        assert v.shape == (3,) and v.dtype == torch.float32 and bool(torch.isfinite(v).all())
    assert torch.equal(rep["mel_distance"], m.round_trip_mel_distance(wavs, bandwidth_id=bw))
    assert torch.equal(rep["stoi"], m.round_trip_stoi(wavs, bandwidth_id=bw))
    assert torch.equal(rep["estoi"], m.round_trip_stoi(wavs, bandwidth_id=bw, extended=True))
    assert torch.equal(rep["stft_distance"], metrics.stft_distance_many(crops, wavs))
    assert torch.equal(rep["si_sdr"], metrics.si_sdr_many(crops, wavs))
    assert torch.equal(rep["snr"], metrics.snr_many(crops, wavs))
    assert "estoi" not in m.round_trip_report(wavs, bandwidth_id=bw)
    assert all(v.shape == (0,) for v in m.round_trip_report([], bandwidth_id=bw).values())


def test_one_pair_is_capturable_in_a_graph():
    """Up to 64 descriptors travel in the launches' argument blocks: no copy and no host wait, so the calls can be captured."""
    from wavtokenizer_amd import metrics
    x, y = _pair(0)
    eager = (metrics.stft_distance(x, y), metrics.si_sdr(x, y, zero_mean=True), metrics.snr(x, y))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.stft_distance(x, y)                                   # (warm-up on the capture stream)
        metrics.si_sdr(x, y, zero_mean=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = (metrics.stft_distance(x, y), metrics.si_sdr(x, y, zero_mean=True), metrics.snr(x, y))
    for t in got:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, eager))
    # the graph reads the inputs where they are: new contents, new result, the bits of the eager call on them
    x2, y2 = _pair(4)
    x.copy_(x2)
    y.copy_(y2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], metrics.stft_distance(x, y)) and torch.equal(got[1], metrics.si_sdr(x, y, zero_mean=True))
    assert not torch.equal(got[0], eager[0])
