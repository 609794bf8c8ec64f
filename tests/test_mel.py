"""The Python surface of the mel metric (wavtokenizer_amd/metrics.py) and WavTokenizer.round_trip_mel_distance on the GPU."""
import numpy as np
import pytest
import torch

from tests import mel_ref as R
from tests.util import synth_state_dict

pytestmark = pytest.mark.gpu


def _clip(name, T, seed=0):
    return torch.from_numpy(R.signal(name, T, seed=seed)).cuda()


def test_shapes_for_the_three_input_ranks():
    from wavtokenizer_amd import metrics
    x = torch.stack([_clip("noise", 3000, seed=s) for s in range(3)])
    one = metrics.mel_spectrogram(x[0])
    two = metrics.mel_spectrogram(x)
    three = metrics.mel_spectrogram(x[:, None, :])
    assert one.shape == (100, 12) and two.shape == (3, 100, 12) and three.shape == (3, 1, 100, 12)
    assert one.dtype == torch.float32 and torch.equal(two[0], one) and torch.equal(three[:, 0], two)
    lin = metrics.mel_spectrogram(x, log=False, hop_length=100, n_mels=64, sample_rate=16000)
    assert lin.shape == (3, 64, 31) and float(lin.min()) >= 0.0
    M64 = R.mel64(x[1].cpu().numpy(), 16000, 100, 64)[0]
    assert np.allclose(lin[1].cpu().numpy(), M64, rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError):
        metrics.mel_spectrogram(x[:, :512])
    with pytest.raises(ValueError):
        metrics.mel_spectrogram(torch.zeros(2, 2, 3000, device="cuda"))


def test_many_equals_the_one_clip_calls_bit_for_bit():
    from wavtokenizer_amd import metrics
    clips = [_clip("noise", 3000), _clip("sine_noise", 8453), _clip("quiet", 513), _clip("burst", 1025)]
    many = metrics.mel_spectrogram_many(clips)
    assert [tuple(m.shape) for m in many] == [(100, 12), (100, 34), (100, 3), (100, 5)]
    base = many[0].untyped_storage().data_ptr()
    assert all(m.untyped_storage().data_ptr() == base for m in many)          # views of one flat tensor
    for m, c in zip(many, clips):
        assert torch.equal(m, metrics.mel_spectrogram(c))
    assert metrics.mel_spectrogram_many([]) == []
    others = [_clip("noise", 3000, seed=3), _clip("sine", 8453), _clip("quiet", 513, seed=3), _clip("noise", 1025, seed=3)]
    d = metrics.mel_distance_many(clips, others)
    assert d.shape == (4,) and d.dtype == torch.float32 and bool(torch.isfinite(d).all())
    for i in range(4):
        assert torch.equal(d[i], metrics.mel_distance_many([clips[i]], [others[i]])[0])
    assert metrics.mel_distance_many([], []).shape == (0,)
    with pytest.raises(ValueError):
        metrics.mel_distance_many(clips[:1], others[1:2])


def test_mel_distance_is_the_mean_of_the_per_clip_distances():
    from wavtokenizer_amd import metrics
    y = torch.stack([_clip("noise", 3000, seed=s) for s in range(3)])
    y_hat = y + 0.01 * torch.stack([_clip("noise", 3000, seed=10 + s) for s in range(3)])
    d = metrics.mel_distance(y_hat, y)
    per = metrics.mel_distance_many(list(y_hat), list(y))
    assert d.dim() == 0 and torch.equal(d, per.mean())
    assert torch.equal(metrics.mel_distance(y_hat[:, None], y[:, None]), d)
    # equal lengths: the reference's l1_loss mean over the whole batch, here from the float64 definition
    want = np.mean([R.distance64(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(y_hat, y)])
    assert abs(float(d) - want) <= 1e-4 * want
    assert float(metrics.mel_distance(y, y)) == 0.0


def test_round_trip_mel_distance():
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer, metrics, synth
    sd = synth_state_dict("hop600")
    m = WavTokenizer.from_arch(ARCH_HOP600)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    m = m.eval().to("cuda")
    wavs = [torch.from_numpy(synth.make_clips(1, T, seed=40 + i)[0]).cuda() for i, T in enumerate((12000, 19999, 28800))]
    bw = torch.tensor([0])
    d = m.round_trip_mel_distance(wavs, bandwidth_id=bw)
    assert d.shape == (3,) and d.dtype == torch.float32 and bool(torch.isfinite(d).all()) and float(d.min()) > 0
    codes = m.encode_codes_many(wavs, bandwidth_id=bw)
    outs = m.decode_codes_many(codes, bandwidth_id=bw)
    by_hand = metrics.mel_distance_many([o[0, :w.shape[0]] for o, w in zip(outs, wavs)], wavs)
    assert torch.equal(d, by_hand)
    assert m.round_trip_mel_distance([], bandwidth_id=bw).shape == (0,)
    d64 = m.round_trip_mel_distance(wavs, bandwidth_id=bw, n_mels=64, hop_length=100)
    assert d64.shape == (3,) and bool(torch.isfinite(d64).all())
    try:
        m.set_gemm_precision("f16")
        d16 = m.round_trip_mel_distance(wavs, bandwidth_id=bw)
    finally:
        m.set_gemm_precision("f16x3")
    assert d16.shape == (3,)
    print(f"round_trip_mel_distance (synthetic hop-600 weights): f16x3 {d.tolist()}  f16 {d16.tolist()}")      # recorded, not asserted
