"""Rows, destinations, the composition and the float64 reference for the ragged emit kernel (csrc/audio.hip emit_kernel, wt_emit)
and for WavTokenizer.decode_pcm / decode_pcm_many: tests/test_emit_op.py and tests/test_decode_pcm.py share them.

The float64 evaluation is the polyphase sum itself, y[n] = sum_k kern[n % new][k] * xpad[(n // new) * orig + k], over
oracle.audio_ref.resample_kernel's float64 table for codec rate -> target rate.  The bound on an fp32 evaluation of that sum is the
one tests/ingest_ref.py derives, (K + 3) * 2^-24 * sum_k |kern_k| |x_k|: a K-term dot product accumulated in fp32 (each of the K
fused multiply-adds rounds once: gamma_K) plus the rounding of the table to fp32 and of its float64 construction (the + 3);
derived, not measured.  At equal rates the kernel copies (K = 1, tap 1.0): the output is the input."""
import ctypes
import math

import numpy as np
import torch

CODEC_RATE = 24000

# (target rate, channels, layout, sample type, n_in, n_out); layout of a stereo clip: "planar" (C, T) or "interleaved" (T, C)
CLIPS = [(16000, 1, "mono", "f32", 9000, 6000),
         (22050, 2, "interleaved", "i16", 7001, 6433),
         (24000, 1, "mono", "i16", 5000, 5000),
         (44100, 2, "planar", "f32", 30011, 55146),
         (48000, 1, "mono", "i16", 2049, 4098),
         (11025, 2, "interleaved", "i16", 4000, 1838),   # orig = 320
         (8000, 1, "mono", "f32", 350, 117),
         (32000, 2, "planar", "f32", 1, 2),
         (25700, 1, "mono", "f32", 1200, 1285)]          # new = 257 > 256: a block spans less than one input period
EDGES = [(16000, 1, "mono", "f32", 383, 256),
         (22050, 2, "interleaved", "i16", 279, 257),
         (24000, 1, "mono", "i16", 257, 257),
         (44100, 2, "planar", "f32", 139, 256)]
HOT_ROW = 1              # the row scaled by 1.3 on top of the 0.9; make_clips stays within about +-0.4, so this clip is emitted with
HOT_LIMIT = 0.25         # limit 0.25, which its samples pass on both sides (the test asserts it); every other int16 clip with
LIMIT = 0.99             # save_audio's default
SENTINEL_F32 = -12345.5
SENTINEL_I16 = -21846    # 0xAAAA


def out_length(rate, n_in):
    return math.ceil(rate * n_in / CODEC_RATE)


def limit_of(j, hot=HOT_ROW):
    return HOT_LIMIT if j == hot else LIMIT


def make_rows(table, behind, seed=40, hot=HOT_ROW):
    """The source rows as the decode plans leave them: [B][pitch] fp32 on the GPU, row j = synth.make_clips(1, n_in_j) * 0.9 (row
    `hot` * 1.3 on top), `behind` in every column from n_in_j on (the pitch leaves at least 33 such columns)."""
    from wavtokenizer_amd import synth
    pitch = max(t[4] for t in table) + 33
    rows = np.full((len(table), pitch), behind, np.float32)
    for j, t in enumerate(table):
        x = synth.make_clips(1, t[4], seed=seed + j)[0] * np.float32(0.9)
        rows[j, :t[4]] = x * np.float32(1.3) if j == hot else x
    return torch.from_numpy(rows).cuda()


class Dest:
    """Where one clip goes: sample (c, n) is buf.view(-1)[off + c * cs + n * ss]."""

    def __init__(self, buf, off, cs, ss, channels, n_out):
        self.buf, self.off, self.cs, self.ss, self.channels, self.n_out = buf, int(off), int(cs), int(ss), int(channels), int(n_out)

    @classmethod
    def of_view(cls, view, channels_last):
        """A 2-D view (C, T) or, with channels_last, (T, C) of some storage, through its own strides."""
        T, C = (view.shape[0], view.shape[1]) if channels_last else (view.shape[1], view.shape[0])
        ss, cs = (view.stride(0), view.stride(1)) if channels_last else (view.stride(1), view.stride(0))
        base = torch.empty(0, dtype=view.dtype, device=view.device).set_(view.untyped_storage())
        return cls(base, view.storage_offset(), cs, ss, C, T)

    def index(self):
        n = torch.arange(self.n_out, device=self.buf.device)
        return torch.stack([self.off + c * self.cs + n * self.ss for c in range(self.channels)])

    def read(self):
        return self.buf.view(-1)[self.index()]               # (channels, n_out)


def strides(layout, n_out, mono_stride=1):
    """(ch_stride, sample_stride, elements spanned) of a clip stored in its table layout."""
    if layout == "mono":
        return 0, mono_stride, (n_out - 1) * mono_stride + 1
    return (1, 2, 2 * n_out) if layout == "interleaved" else (n_out, 1, 2 * n_out)


def lay_out(table, parity=None, mono_stride=None):
    """Destinations for the table in two flat buffers, fp32 and int16, each pre-filled with its sentinel, with padding before,
    between and behind the clips.  parity[j] (0 / 1) is the parity of clip j's first element (default: alternating per buffer,
    starting even, so that int16 pairs and interleaved frames meet both alignments); mono_stride[j] the sample stride of a mono
    clip."""
    cursor = {"f32": 5, "i16": 3}
    count = {"f32": 0, "i16": 0}
    plan = []
    for j, (rate, ch, layout, kind, _n_in, n_out) in enumerate(table):
        cs, ss, span = strides(layout, n_out, (mono_stride or {}).get(j, 1))
        want = parity[j] if parity is not None and parity[j] is not None else count[kind] % 2
        off = cursor[kind] + (cursor[kind] % 2 != want)
        plan.append((kind, off, cs, ss, ch, n_out))
        cursor[kind] = off + span + 5
        count[kind] += 1
    bufs = {"f32": torch.full((cursor["f32"] + 9,), SENTINEL_F32, dtype=torch.float32, device="cuda"),
            "i16": torch.full((cursor["i16"] + 9,), SENTINEL_I16, dtype=torch.int16, device="cuda")}
    return [Dest(bufs[k], off, cs, ss, ch, n) for k, off, cs, ss, ch, n in plan], bufs


def untouched(buf, dests, sentinel):
    """Whether every element of buf outside the dests' spans still holds the sentinel."""
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    for d in dests:
        if d.buf is buf:
            mask[d.index().view(-1)] = False
    return bool((buf.view(-1)[mask] == sentinel).all())


def emit(rows, n_in, rates, dests, limits):
    """One wt_emit launch: row j (a 1-D fp32 view on the GPU, read up to n_in[j]) to dests[j] at rates[j]; the destination's dtype
    decides the sample type.  Waits for it and returns the workspace, filled with 0xAB before the launch, as (the
    wt_emit_workspace_bytes(B) bytes, the 64 bytes behind them)."""
    from wavtokenizer_amd import _capi, audio
    dev = torch.cuda.current_device()
    B = len(rows)
    descs = (_capi.WtEmitClip * B)()
    for d, row, n, rate, dst, lim in zip(descs, rows, n_in, rates, dests, limits):
        d.src, d.n_in, d.resampler = row.data_ptr(), n, audio.resampler(CODEC_RATE, rate, dev)
        d.n_out = out_length(rate, n)
        assert d.n_out == dst.n_out
        d.dst = dst.buf.data_ptr() + dst.off * dst.buf.element_size()
        d.dtype = _capi.WT_EMIT_I16 if dst.buf.dtype == torch.int16 else _capi.WT_EMIT_F32
        d.channels, d.ch_stride, d.sample_stride, d.limit = dst.channels, dst.cs, dst.ss, lim
    nbytes = int(_capi.lib.wt_emit_workspace_bytes(B))
    ws = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(_capi.lib.wt_emit(descs, B, ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                "wt_emit")
    torch.cuda.synchronize()
    return ws[:nbytes], ws[nbytes:]


def composition(row, rate, kind="f32", limit=LIMIT):
    """What the caller did by hand: audio.convert_audio of the clip alone (a copy of its n_in samples) and, for int16,
    audio.to_pcm16: 1-D on the GPU."""
    from wavtokenizer_amd import audio
    r = audio.convert_audio(row.clone()[None, None], CODEC_RATE, rate, 1)[0, 0]
    return audio.to_pcm16(r, limit=limit) if kind == "i16" else r


def pcm16_numpy(x, limit):
    """to_pcm16 without rescale in numpy on fp32 values: clamp, x * 32768 (exact in fp32), round half to even, clip."""
    x = np.asarray(x, np.float32)
    v = np.clip(x, np.float32(-limit), np.float32(limit)) * np.float32(32768.0)
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def ref64(row, rate):
    """(y, bound) in float64 for one row (numpy fp32, n_in samples) resampled from the codec rate to `rate`."""
    from oracle.audio_ref import resample_kernel
    x = np.asarray(row, np.float32)
    T = x.shape[0]
    if rate == CODEC_RATE:
        y = x.astype(np.float64)
        return y, 4 * 2.0 ** -24 * np.abs(y)
    kern, width, orig, new = resample_kernel(CODEC_RATE, rate)
    K = kern.shape[1]
    n_out = out_length(rate, T)
    nfr = -(-n_out // new)
    xpad = np.zeros(width + nfr * orig + K, np.float64)
    xpad[width:width + T] = x
    frames = np.lib.stride_tricks.sliding_window_view(xpad, K)[::orig][:nfr]          # [frames][K]
    y = np.einsum("fk,pk->fp", frames, kern).reshape(-1)[:n_out]
    absum = np.einsum("fk,pk->fp", np.abs(frames), np.abs(kern)).reshape(-1)[:n_out]
    return y, (K + 3) * 2.0 ** -24 * absum


def pcm_composition(model, codes, rate, channels, dtype, channels_last, limit, bw):
    """decode_pcm_many's clip by hand over decode_codes: (channels, n_out) or (n_out, channels)."""
    from wavtokenizer_amd import audio
    r = audio.convert_audio(model.decode_codes(codes, bandwidth_id=bw)[:, None], CODEC_RATE, rate, 1)[0]      # (1, n_out)
    if dtype == torch.int16:
        r = audio.to_pcm16(r, limit=limit)
    r = r.expand(channels, -1)
    return r.t().contiguous() if channels_last else r.contiguous()
