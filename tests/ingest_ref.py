"""Clips, the composition and the float64 reference for the ragged ingest kernel (csrc/audio.hip ingest_kernel) and for
WavTokenizer.encode_codes_many: tests/test_ingest_op.py and tests/test_encode_codes.py share them.

The float64 evaluation is the polyphase sum itself, y[n] = sum_k kern[n % new][k] * xpad[(n // new) * orig + k], over
oracle.audio_ref.resample_kernel's float64 table and the fp32 channel mean (the mean of two fp32 values is rounded once, as
the kernel rounds it; the int16 scaling by 1 / 32768 is exact).  The bound on an fp32 evaluation of that sum,
(K + 3) * 2^-24 * sum_k |kern_k| |x_k|, is the standard bound of a K-term dot product accumulated in fp32 (each of the K fused
multiply-adds rounds once: gamma_K) plus the rounding of the table to fp32 and of its float64 construction (the + 3); it is
derived, not measured."""
import math

import numpy as np
import torch

CODEC_RATE = 24000

# (source rate, channels, layout, sample type, samples per channel); layout of a stereo clip: "planar" (C, T) or
# "interleaved" (T, C); mono clips are 1-D
CLIPS = [(16000, 1, "mono", "f32", 9000),
         (22050, 2, "interleaved", "i16", 7001),
         (24000, 1, "mono", "i16", 5000),
         (44100, 2, "planar", "f32", 30011),
         (48000, 1, "mono", "i16", 2049),
         (11025, 2, "interleaved", "i16", 4000),     # nw = 320 > 256: a block spans less than one input period
         (8000, 1, "mono", "f32", 350),
         (32000, 2, "planar", "f32", 1)]
EDGE_N_IN = [255, 256, 257, 147]                     # the first four clips again, around the block edges


def make_clip(rate, channels, layout, kind, n_in, seed):
    """One clip on the CPU in its own layout and sample type: synth.make_clips(channels, n_in, seed) scaled by 0.9, rounded to
    int16 for an int16 clip."""
    from wavtokenizer_amd import synth
    x = synth.make_clips(channels, n_in, seed=seed, sample_rate=rate) * np.float32(0.9)
    if kind == "i16":
        x = np.rint(x * np.float32(32768.0)).clip(-32768, 32767).astype(np.int16)
    t = torch.from_numpy(x)
    if layout == "mono":
        return t[0].clone()
    return t.t().contiguous() if layout == "interleaved" else t


def table_clips(n_in=None):
    """[(clip, rate, layout)] of the table above (seed 20 + i), optionally with other lengths for the first len(n_in) clips."""
    rows = CLIPS if n_in is None else [c[:4] + (n,) for c, n in zip(CLIPS, n_in)]
    return [(make_clip(*row, seed=20 + i), row[0], row[2]) for i, row in enumerate(rows)]


def planar_f32(clip, layout):
    """The clip as the composition feeds it to convert_audio: (C, T) fp32, an int16 clip divided by 32768."""
    x = clip.float() / 32768 if clip.dtype == torch.int16 else clip
    if layout == "mono":
        return x[None]
    return x.t() if layout == "interleaved" else x


def out_length(rate, n_in):
    return math.ceil(CODEC_RATE * n_in / rate)


def ref64(planar, rate):
    """(y, bound) in float64 for one clip (C, T) fp32 (numpy): the polyphase sum over the float64 table and the fp32 channel
    mean, and the bound of its fp32 evaluation per output."""
    from oracle.audio_ref import resample_kernel
    x = np.asarray(planar, np.float32)
    mono = x[0] if x.shape[0] == 1 else ((x[0] + x[1]) * np.float32(0.5)).astype(np.float32)
    T = mono.shape[0]
    if rate == CODEC_RATE:
        y = mono.astype(np.float64)
        return y, 4 * 2.0 ** -24 * np.abs(y)
    kern, width, orig, new = resample_kernel(rate, CODEC_RATE)
    K = kern.shape[1]
    n_out = out_length(rate, T)
    nfr = -(-n_out // new)
    xpad = np.zeros(width + nfr * orig + K, np.float64)
    xpad[width:width + T] = mono
    frames = np.lib.stride_tricks.sliding_window_view(xpad, K)[::orig][:nfr]          # [frames][K]
    y = np.einsum("fk,pk->fp", frames, kern).reshape(-1)[:n_out]
    absum = np.einsum("fk,pk->fp", np.abs(frames), np.abs(kern)).reshape(-1)[:n_out]
    return y, (K + 3) * 2.0 ** -24 * absum


def ingest(model, clips, rates, layouts, T_pad=None, sentinel=None):
    """One wt_ingest launch over the clips through the model's own staging (WavTokenizer._ingest_stage): returns the staging
    tensor [B][T_pad] (pre-filled with the sentinel where one is given) and the clips' output lengths."""
    from wavtokenizer_amd import _capi, pretrained
    dev = torch.device("cuda", torch.cuda.current_device())
    specs = []
    for c, sr, lay in zip(clips, rates, layouts):
        ch = 1 if c.dim() == 1 else int(c.shape[1 if lay == "interleaved" else 0])
        n_in = int(c.shape[0]) if c.dim() == 1 or lay == "interleaved" else int(c.shape[1])
        specs.append(pretrained._ClipSpec(c, ch, n_in, lay == "interleaved", sr, out_length(sr, n_in)))
    n_out = [sp.n_out for sp in specs]
    T_pad = T_pad or max(n_out)
    descs, ws, lengths, spans, _alive = model._ingest_stage(specs, [0] * len(specs), dev)
    out = torch.empty((len(specs), T_pad), dtype=torch.float32, device=dev)
    if sentinel is not None:
        out.fill_(sentinel)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(_capi.lib.wt_ingest(descs, len(specs), T_pad, out.data_ptr(), ws.data_ptr(), stream), "wt_ingest")
    torch.cuda.current_stream(dev).synchronize()
    assert lengths.tolist() == n_out
    return out, n_out
