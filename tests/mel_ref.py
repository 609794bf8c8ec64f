"""The mel spectrogram and distance of csrc/mel.hip (include/wavtokenizer_amd.h gives the definition) in float64 numpy, an fp32
stand-in of the same pipeline with a plain radix-2 FFT that serves as the yardstick for the kernel's rounding error, the error
statistic and the bounds derived from it, and the signals and ctypes plumbing the mel tests share.  Written from the definition
(what torchaudio.transforms.MelSpectrogram(sample_rate, n_fft=1024, hop_length, n_mels, center=True, power=1) computes with its
defaults); torchaudio is not available here, so the parity with it is unpinned."""
import functools

import numpy as np

N_FFT = 1024
BINS = N_FFT // 2 + 1
FLOOR = 1e-7
EPS32 = 2.0 ** -23


def window64():
    """The periodic Hann window [1024] in float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)


@functools.lru_cache(maxsize=None)
def tables(sample_rate: int, n_mels: int):
    """(window [1024], fb [513][n_mels]) in float64."""
    window = window64()
    all_freqs = np.linspace(0, sample_rate // 2, BINS)
    m_max = 2595.0 * np.log10(1.0 + (sample_rate / 2.0) / 700.0)
    m_pts = np.linspace(0.0, m_max, n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]                     # [513][n_mels + 2]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    return window, fb


def empty_filters(sample_rate: int, n_mels: int):
    """The filters without a single bin in the table a handle uploads (the float64 definition rounded once to fp32): the two
    edges of a narrow low filter can fall between two bins of the 513."""
    fb32 = tables(sample_rate, n_mels)[1].astype(np.float32)
    return np.nonzero((fb32 != 0).sum(axis=0) == 0)[0]


def n_frames(T: int, hop: int) -> int:
    return 1 + T // hop


def frames64(x, hop: int):
    """The windowed frames [F][1024] of a clip in float64: reflect padding by 512, frame f starts at f * hop."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 1 and x.shape[0] > N_FFT // 2
    xp = np.pad(x, N_FFT // 2, mode="reflect")
    F = n_frames(x.shape[0], hop)
    idx = np.arange(F)[:, None] * hop + np.arange(N_FFT)[None, :]
    return xp[idx] * window64()[None, :]


def frame_support(T: int, hop: int):
    """[F][1024] indices into the clip of every frame's samples, reflection included."""
    idx = np.pad(np.arange(T), N_FFT // 2, mode="reflect")
    return idx[np.arange(n_frames(T, hop))[:, None] * hop + np.arange(N_FFT)[None, :]]


def mel64(x, sample_rate=24000, hop=256, n_mels=100):
    """(M [n_mels][F], norms [F]): the linear mel spectrogram in float64 and the 2-norm of every windowed frame."""
    fr = frames64(x, hop)
    S = np.abs(np.fft.rfft(fr, axis=1))                               # [F][513]
    M = tables(sample_rate, n_mels)[1].T @ S.T
    return M, np.sqrt((fr * fr).sum(axis=1))


def safe_log(M):
    return np.log(np.maximum(M, FLOOR))


def distance64(a, b, sample_rate=24000, hop=256, n_mels=100) -> float:
    return float(np.abs(safe_log(mel64(a, sample_rate, hop, n_mels)[0]) - safe_log(mel64(b, sample_rate, hop, n_mels)[0])).mean())


def _bitrev(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])


def standin_fp32(x, sample_rate=24000, hop=256, n_mels=100):
    """The same pipeline in float32 throughout with a plain radix-2 decimation-in-time complex FFT of the 1024 windowed samples
    (zero imaginary part): window, twiddles and filters rounded once from float64, every product and sum rounded to float32.
    Returns M [n_mels][F] float32."""
    f32 = np.float32
    x = np.asarray(x, f32)
    window, fb = tables(sample_rate, n_mels)
    xp = np.pad(x, N_FFT // 2, mode="reflect")
    F = n_frames(x.shape[0], hop)
    idx = np.arange(F)[:, None] * hop + np.arange(N_FFT)[None, :]
    re = (xp[idx] * window.astype(f32)[None, :])[:, _bitrev(N_FFT)].astype(f32)
    im = np.zeros_like(re)
    half = 1
    while half < N_FFT:
        ang = -np.pi * np.arange(half, dtype=np.float64) / half
        wr, wi = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
        re = re.reshape(F, -1, 2, half)
        im = im.reshape(F, -1, 2, half)
        tr = (re[:, :, 1] * wr - im[:, :, 1] * wi).astype(f32)
        ti = (re[:, :, 1] * wi + im[:, :, 1] * wr).astype(f32)
        re = np.stack([re[:, :, 0] + tr, re[:, :, 0] - tr], axis=2).astype(f32).reshape(F, N_FFT)
        im = np.stack([im[:, :, 0] + ti, im[:, :, 0] - ti], axis=2).astype(f32).reshape(F, N_FFT)
        half *= 2
    S = np.sqrt((re[:, :BINS] * re[:, :BINS] + im[:, :BINS] * im[:, :BINS]).astype(f32)).astype(f32)      # [F][513]
    fb32 = fb.astype(f32)
    M = np.zeros((n_mels, F), f32)
    for k in range(BINS):                                             # ascending bins, one rounded product and sum each
        M = (M + (fb32[k][:, None] * S[:, k][None, :]).astype(f32)).astype(f32)
    return M


def scale64(M64, norms, sample_rate=24000, n_mels=100):
    """The condition of a mel entry: ||fb[:, m]||_1 ||w x_f||_2 + M64.  FFT rounding is relative to the frame's energy, not to the
    bin, and a filter adds up |fb|-weighted bins."""
    fb = tables(sample_rate, n_mels)[1]
    return np.abs(fb).sum(axis=0)[:, None] * norms[None, :] + M64


def error_stat(M, M64, norms, sample_rate=24000, n_mels=100) -> float:
    """r = max |M - M64| / (2^-23 (||fb[:, m]||_1 ||w x_f||_2 + M64)); 0 for a clip of zeros that comes out as zeros."""
    err = np.abs(np.asarray(M, np.float64) - M64)
    sc = EPS32 * scale64(M64, norms, sample_rate, n_mels)
    ok = sc > 0
    assert bool((err[~ok] == 0).all())
    return float((err[ok] / sc[ok]).max()) if ok.any() else 0.0


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def log_bound(bar: float, M64, norms, sample_rate=24000, n_mels=100):
    """(bound on |L - L64| per entry, entries that may be left out): with b = bar 2^-23 scale the linear bound, |log(M64 +- b) -
    log M64| <= b / M64 (1 + b / M64) while b < M64 / 2, plus 2 ulp for the fp32 log and the rounding of its result.  The clip at
    1e-7 moves no two values apart, so below it M64 stands for max(M64, 1e-7): a frame of zeros (b = 0) is held to the 2 ulp."""
    b = bar * EPS32 * scale64(M64, norms, sample_rate, n_mels)
    q = b / np.maximum(M64, FLOOR)
    skip = ~(q < 0.5)
    bound = np.where(skip, np.inf, q * (1 + q)) + 2 * ulp32(safe_log(M64))
    return bound, skip


def _wave_sum(v):
    """The xor butterfly of a wave over v [..., 64] float32 (offsets 32, 16, ..., 1, every lane adds its partner's value): lane 0."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ off]).astype(np.float32)
    return v[..., 0]


def distance_fp32(La, Lb) -> np.float32:
    """The distance kernels' arithmetic on two fp32 log-mel spectrograms [n_mels][F], rounding for rounding (csrc/mel.hip
    mel_block and mel_mean_block): per frame lane l adds |La - Lb| of filters l and l + 64 (0 where there is none), the xor
    butterfly adds the lanes; per clip lane l adds partials l, l + 64, ... in ascending order from 0, the butterfly again, one
    division by float(n_mels) * float(F)."""
    f32 = np.float32
    La, Lb = np.asarray(La, f32), np.asarray(Lb, f32)
    n_mels, F = La.shape
    d = np.zeros((128, F), f32)
    d[:n_mels] = np.abs((La - Lb).astype(f32))
    part = _wave_sum((d[:64] + d[64:]).astype(f32).T)                # [F]
    padded = np.zeros(-(-F // 64) * 64, f32)
    padded[:F] = part
    s = np.zeros(64, f32)
    for row in padded.reshape(-1, 64):                               # (a lane past F adds nothing in the kernel; + 0 changes no bit)
        s = (s + row).astype(f32)
    return f32(_wave_sum(s) / (f32(n_mels) * f32(F)))


# ------------------------------------------------------------------------------------------------ signals
SIGNALS = ("noise", "quiet", "sine_noise", "sine", "dc", "square", "burst")
BROADBAND = ("noise", "quiet", "sine_noise", "burst")
LENGTHS = (513, 768, 1023, 1024, 1025, 3000, 8453)


def signal(name: str, T: int, seed: int = 0, sample_rate: int = 24000):
    rng = np.random.default_rng(1000 * seed + T)
    t = np.arange(T, dtype=np.float64) / sample_rate
    if name == "noise":
        x = 0.1 * rng.standard_normal(T)
    elif name == "quiet":
        x = 3e-4 * rng.standard_normal(T)
    elif name == "sine_noise":
        x = 0.5 * np.sin(2 * np.pi * 440.0 * t) + 1e-3 * rng.standard_normal(T)
    elif name == "sine":
        x = 0.5 * np.sin(2 * np.pi * 440.0 * t)
    elif name == "dc":
        x = np.full(T, 0.25)
    elif name == "square":
        x = 0.9 * np.sign(np.sin(2 * np.pi * 300.0 * t) + 1e-12)
    elif name == "burst":
        x = np.zeros(T)
        x[T - 200:] = 0.1 * rng.standard_normal(200)
    elif name == "silence":
        x = np.zeros(T)
    else:
        raise KeyError(name)
    return x.astype(np.float32)


def noisy_pair(T: int):
    """Noise and a copy of it with noise 40 dB below added: the pair of a distance near 0.005."""
    a = signal("noise", T, seed=1)
    return a, (a + 1e-3 * np.random.default_rng(T).standard_normal(T)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the calls, through ctypes
CANARY = 12345.0


class Arena:
    """Clips in one NaN-filled device buffer, NaN directly before and after every clip (a read outside [0, T) poisons the
    output), at odd element offsets."""

    def __init__(self, clips):
        import torch
        self.off, cur = [], 3
        for c in clips:
            self.off.append(cur)
            cur += len(c) + 5
        host = np.full(cur + 3, np.nan, np.float32)
        for o, c in zip(self.off, clips):
            host[o:o + len(c)] = c
        self.buf = torch.from_numpy(host).cuda()
        self.len = [len(c) for c in clips]

    def ptr(self, i):
        return self.buf.data_ptr() + 4 * self.off[i]


class Outputs:
    """Outputs of given sizes in one device buffer with canaries around each."""

    def __init__(self, sizes):
        import torch
        self.off, cur = [], 7
        for s in sizes:
            self.off.append(cur)
            cur += s + 7
        self.sizes = list(sizes)
        self.buf = torch.full((cur,), CANARY, dtype=torch.float32, device="cuda")

    def ptr(self, i):
        return self.buf.data_ptr() + 4 * self.off[i]

    def read(self):
        """(outputs as float32 numpy arrays, whether every word outside them still holds the canary)."""
        host = self.buf.cpu().numpy()
        mask = np.ones(host.shape[0], bool)
        outs = []
        for o, s in zip(self.off, self.sizes):
            outs.append(host[o:o + s].copy())
            mask[o:o + s] = False
        return outs, bool((host[mask] == np.float32(CANARY)).all())


@functools.lru_cache(maxsize=None)
def handle(sample_rate=24000, hop=256, n_mels=100):
    from wavtokenizer_amd import metrics
    return metrics.mel_handle(sample_rate, N_FFT, hop, n_mels, 0)


def run(clips_a, clips_b=None, log=True, sample_rate=24000, hop=256, n_mels=100, ws_fill=0xAB, with_workspace=False):
    """One wt_mel_spectrogram (clips_b None) or wt_mel_distance call on clips laid out in a NaN arena, outputs between canaries,
    the workspace filled with ws_fill beforehand.  Returns (outputs: [n_mels][F] arrays or floats, canaries intact) and, with
    with_workspace, the workspace's bytes after the call as a third item."""
    import ctypes

    import torch

    from wavtokenizer_amd._capi import WtMelClip, check, lib
    n = len(clips_a)
    dist = clips_b is not None
    arena = Arena(list(clips_a) + (list(clips_b) if dist else []))
    F = [n_frames(len(c), hop) for c in clips_a]
    outs = Outputs([1] * n if dist else [n_mels * f for f in F])
    nbytes = int(lib.wt_mel_workspace_bytes(n, sum(F) if dist else 0))
    ws = torch.full((nbytes + 64,), ws_fill, dtype=torch.uint8, device="cuda")
    descs = (WtMelClip * n)()
    for i in range(n):
        descs[i].a = arena.ptr(i)
        descs[i].b = arena.ptr(n + i) if dist else None
        descs[i].length = len(clips_a[i])
        descs[i].out = outs.ptr(i)
    h = handle(sample_rate, hop, n_mels)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if dist:
        check(lib.wt_mel_distance(h, descs, n, ctypes.c_void_p(ws.data_ptr()), stream), "wt_mel_distance")
    else:
        check(lib.wt_mel_spectrogram(h, descs, n, 1 if log else 0, ctypes.c_void_p(ws.data_ptr()), stream), "wt_mel_spectrogram")
    torch.cuda.synchronize()
    got, intact = outs.read()
    assert bool((ws[nbytes:] == ws_fill).all()), "the call wrote behind its workspace"
    res = [g[0] for g in got] if dist else [g.reshape(n_mels, f) for g, f in zip(got, F)]
    return (res, intact, ws[:nbytes].cpu().numpy()) if with_workspace else (res, intact)
