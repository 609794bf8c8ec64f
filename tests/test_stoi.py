"""The Python surface of STOI (wavtokenizer_amd/metrics.py) and WavTokenizer.round_trip_stoi on the GPU."""
import numpy as np
import pytest
import torch

from tests import stoi_ref as R
from tests.util import synth_state_dict

pytestmark = pytest.mark.gpu

# (samples, rate): mixed lengths and mixed rates
PAIRS = [(12000, 24000), (9831, 24000), (9830, 24000), (6554, 16000), (31000, 24000), (4225, 10000), (18064, 44100), (20000, 16000)]


def _pair(i):
    T, fs = PAIRS[i]
    x = R.speechlike(T, fs, seed=50 + i)
    return torch.from_numpy(x).cuda(), torch.from_numpy(R.noisy(x, (20, 0, -10)[i % 3], seed=i)).cuda(), fs


@pytest.fixture(scope="module")
def alone():
    """Every pair's own stoi call, STOI and ESTOI."""
    from wavtokenizer_amd import metrics
    out = []
    for i in range(len(PAIRS)):
        x, y, fs = _pair(i)
        out.append((metrics.stoi(x, y, fs), metrics.stoi(x, y, fs, extended=True)))
    return out


def test_shapes_and_values(alone):
    from wavtokenizer_amd import metrics
    # the bar of the kernel test (tests/test_stoi_op.py), on these pairs: 4 x the worst deviation of the fp32 stand-in from float64,
    # computed here on the CPU, with the same conditions on the pairs asserted first
    refs, worst = [], [0.0, 0.0]
    for i in range(len(PAIRS)):
        x, y, fs = _pair(i)
        s64 = R.stages(x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64), fs)
        assert R.keep_margin(s64) >= 1e-3 and min(s64.cond.values()) >= 1e-3, i
        s32 = R.stages(x.cpu().numpy(), y.cpu().numpy(), fs, np.float32, keep=s64.keep)
        refs.append((float(s64.d[False]), float(s64.d[True])))
        worst = [max(w, abs(float(s32.d[k]) - float(s64.d[k]))) for w, k in zip(worst, (False, True))]
    assert all(0 < w < 1e-4 for w in worst)
    for i, (d, e) in enumerate(alone):
        assert d.dim() == 0 and d.dtype == torch.float32 and d.is_cuda and e.dim() == 0
        want = refs[i]
        print(f"stoi pair {i} {PAIRS[i]}: STOI {float(d):.7f} (float64 {want[0]:.7f}, bar {4 * worst[0]:.2e})  "
              f"ESTOI {float(e):.7f} (float64 {want[1]:.7f}, bar {4 * worst[1]:.2e})")
        assert abs(float(d) - want[0]) <= 4 * worst[0] and abs(float(e) - want[1]) <= 4 * worst[1], (i, float(d), float(e), want, worst)
        if PAIRS[i] == (9830, 24000):
            assert float(d) == float(np.float32(1e-5)) == float(e)
        else:
            assert float(d) != float(e)
    x, y, fs = _pair(0)
    assert float(metrics.stoi(x, x, fs)) > 0.9999 and float(metrics.stoi(x, x, fs, extended=True)) > 0.9999


def test_many_has_the_bits_of_the_one_pair_calls_at_any_position(alone):
    from wavtokenizer_amd import metrics
    n = len(PAIRS)
    pairs = [_pair(i) for i in range(n)]
    # three batches: the eight pairs; reversed; and 40 pairs of one more rate group than fits the launches' argument blocks
    orders = [list(range(n)), list(range(n))[::-1], [i % n for i in range(3, 83)]]
    for order in orders:
        for ext in (False, True):
            d = metrics.stoi_many([pairs[i][0] for i in order], [pairs[i][1] for i in order], sample_rate=[pairs[i][2] for i in order],
                                  extended=ext)
            assert d.shape == (len(order),) and d.dtype == torch.float32
            for pos, i in enumerate(order):
                assert torch.equal(d[pos], alone[i][1 if ext else 0]), (order[:4], pos, i, ext)
    same = [i for i in range(n) if PAIRS[i][1] == 24000]
    d = metrics.stoi_many([pairs[i][0] for i in same], [pairs[i][1] for i in same], sample_rate=24000)
    assert all(torch.equal(d[k], alone[i][0]) for k, i in enumerate(same))
    assert metrics.stoi_many([], []).shape == (0,)
    with pytest.raises(ValueError):
        metrics.stoi_many([pairs[0][0]], [pairs[1][1]])


def test_rows_of_a_batch_equal_the_loop_over_them():
    from wavtokenizer_amd import metrics
    x = torch.stack([torch.from_numpy(R.speechlike(15000, 24000, seed=70 + s)) for s in range(3)]).cuda()
    y = torch.stack([torch.from_numpy(R.noisy(x[s].cpu().numpy(), 5.0 * s, seed=s)) for s in range(3)]).cuda()
    for ext in (False, True):
        d = metrics.stoi(x, y, 24000, extended=ext)
        assert d.shape == (3,)
        for s in range(3):
            assert torch.equal(d[s], metrics.stoi(x[s], y[s], 24000, extended=ext))
        assert torch.equal(metrics.stoi(x[:, None], y[:, None], 24000, extended=ext), d)
    with pytest.raises(ValueError):
        metrics.stoi(x[:, :600], y[:, :600])


def test_round_trip_stoi():
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
    for ext in (False, True):
        d = m.round_trip_stoi(wavs, bandwidth_id=bw, extended=ext)
        assert d.shape == (3,) and d.dtype == torch.float32 and bool(torch.isfinite(d).all())
        assert torch.equal(d, metrics.stoi_many(wavs, crops, sample_rate=24000, extended=ext))
    assert m.round_trip_stoi([], bandwidth_id=bw).shape == (0,)


def test_one_pair_is_capturable_in_a_graph():
    from wavtokenizer_amd import metrics
    x, y, fs = _pair(0)
    eager = metrics.stoi(x, y, fs)
    eager_e = metrics.stoi(x, y, fs, extended=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.stoi(x, y, fs)                                        # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d = metrics.stoi(x, y, fs)
        e = metrics.stoi(x, y, fs, extended=True)
    d.zero_()
    e.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(d, eager) and torch.equal(e, eager_e)
    # the graph reads the inputs where they are: new contents, new result, the bits of the eager call on them
    x2, y2, _ = _pair(4)
    x.copy_(x2[:x.shape[0]])
    y.copy_(y2[:y.shape[0]])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(d, metrics.stoi(x, y, fs)) and not torch.equal(d, eager)
