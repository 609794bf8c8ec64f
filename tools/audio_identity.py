#!/usr/bin/env python3
"""What the loaded library makes of fixed seeded inputs in the ragged audio and metric calls: one sha256 line per case over the raw
bytes of the outputs.  Run it once per library (WAVTOK_HIP_LIB=tools/lib/libwavtok_hip_prev.so for the parent's,
tools/build_prev.sh) and compare the lines: a refactor of csrc/audio.hip, mel.hip or stoi.hip leaves every line as it was.

  mel         linear, log and distance at B = 1, 64, 65 (up to 64 descriptors travel in the kernels' argument block)
  stoi, estoi at 10000 Hz (no resampling), 16000, 24000 and 44100 Hz (its filter is beyond the 48 KiB the LDS form of the resampling
              kernel takes; the tool says which form each rate gets) at B = 1, 32, 33
  stft        distance (with its components) and the magnitudes of each default resolution at B = 1, 64, 65
  wavedist    SI-SDR and SNR (wt_wavedist), with and without zero_mean, at B = 1, 64, 65
  emit        fp32 and int16, mono and stereo, equal rates (the copy form) and 24000 -> 16000 Hz, at B = 64, 65
  overlap-add ragged, at B = 64, 65
  ingest      fp32 and int16 at B = 3"""
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from wavtokenizer_amd import _capi, audio, metrics
from wavtokenizer_amd._capi import _ptr, _stream, check, lib

DEV = torch.device("cuda", 0)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def clips(n, lengths, seed, scale=0.1):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy((scale * rng.standard_normal(lengths[j % len(lengths)])).astype(np.float32)).to(DEV) for j in range(n)]


def mel_cases():
    for B in (1, 64, 65):
        a, b = clips(B, (513, 1300, 1025, 2000), 10 + B), clips(B, (513, 1300, 1025, 2000), 20 + B)
        yield f"mel linear B={B}", sha(*metrics.mel_spectrogram_many(a, log=False))
        yield f"mel log B={B}", sha(*metrics.mel_spectrogram_many(a, log=True))
        yield f"mel distance B={B}", sha(metrics.mel_distance_many(a, b))


def stoi_lds_bytes(rate):
    """stoi_resample_lds_bytes (csrc/stoi.hip) on the host."""
    p, q, L = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    check(lib.wt_stoi_tables(rate, ctypes.byref(p), ctypes.byref(q), ctypes.byref(L), None, None, None), "wt_stoi_tables")
    return 4 * (2 * L.value + 1 + 255 * q.value // p.value + 2 * L.value // p.value + 3)


def stoi_cases():
    for rate in (10000, 16000, 24000, 44100):
        p, q = metrics.stoi_ratio(rate)
        T = -(-4100 * q // p)                                   # 31 candidate frames at 10 kHz
        assert metrics.stoi_frames(T, rate)[1] == 31
        form = "no resampling" if p == q else f"resampling filter {stoi_lds_bytes(rate)} B: {'LDS' if stoi_lds_bytes(rate) <= 48 * 1024 else 'global'} form"
        for B in (1, 32, 33):
            clean = clips(B, (T, T + 37), 30 + B)
            noise = clips(B, (T, T + 37), 40 + B, scale=0.03)
            proc = [c + n for c, n in zip(clean, noise)]
            for ext in (False, True):
                yield f"{'estoi' if ext else 'stoi'} {rate} Hz ({form}) B={B}", sha(metrics.stoi_many(clean, proc, sample_rate=rate, extended=ext))


def stft_cases():
    """(a library from before the STFT distance has none of these entry points: its run prints no such line)"""
    for B in (1, 64, 65):
        a, b = clips(B, (1025, 1300, 2049, 3000), 80 + B), clips(B, (1025, 1300, 2049, 3000), 90 + B)
        d, c = metrics.stft_distance_many(a, b, components=True)
        yield f"stft distance B={B}", sha(d, c)
        for n_fft, hop, win in zip(metrics.STFT_FFT_SIZES, metrics.STFT_HOP_SIZES, metrics.STFT_WIN_LENGTHS):
            yield f"stft magnitude n_fft={n_fft} B={B}", sha(*metrics.stft_magnitude_many(a, n_fft, hop, win))


def wavedist_cases():
    for B in (1, 64, 65):
        a, b = clips(B, (1, 65, 2048, 2049, 7000), 100 + B), clips(B, (1, 65, 2048, 2049, 7000), 110 + B, scale=0.03)
        est = [x + y for x, y in zip(a, b)]
        for zm in (False, True):
            yield f"wavedist zero_mean={int(zm)} B={B}", sha(metrics.wavedist_many(est, a, zero_mean=zm))


def emit_cases():
    for B in (64, 65):
        for rate in (24000, 16000):
            r = audio.resampler(24000, rate, 0)
            n_in = [300 + 7 * (j % 9) for j in range(B)]
            n_out = [int(lib.wt_resampler_out_length(r, n)) for n in n_in]
            rows = clips(B, n_in, 50 + B, scale=0.4)
            for kind, dt in (("fp32", torch.float32), ("int16", torch.int16)):
                for ch in (1, 2):
                    outs = [torch.zeros(n * ch, dtype=dt, device=DEV) for n in n_out]      # stereo: interleaved frames
                    descs = (_capi.WtEmitClip * B)()
                    for d, row, ni, no, o in zip(descs, rows, n_in, n_out, outs):
                        d.src, d.n_in, d.resampler, d.n_out, d.dst = row.data_ptr(), ni, r, no, o.data_ptr()
                        d.dtype = _capi.WT_EMIT_I16 if dt == torch.int16 else _capi.WT_EMIT_F32
                        d.channels, d.ch_stride, d.sample_stride, d.limit = ch, ch - 1, ch, 0.25
                    ws = torch.empty(int(lib.wt_emit_workspace_bytes(B)), dtype=torch.uint8, device=DEV)
                    check(lib.wt_emit(descs, B, _ptr(ws), _stream(DEV)), "wt_emit")
                    yield f"emit {kind} {'stereo' if ch == 2 else 'mono'} 24000 -> {rate} B={B}", sha(*outs)


def overlap_add_cases():
    cases = [(8, 3, 17), (8, 8, 24), (257, 100, 999), (64, 48, 300)]           # (frame_len, stride, total)
    for B in (64, 65):
        rng = np.random.default_rng(60 + B)
        keep, descs, outs = [], (_capi.WtOverlapAddClip * B)(), []
        for j, d in enumerate(descs):
            flen, stride, total = cases[j % len(cases)]
            nf = (total - 1) // stride + 1
            frames = torch.from_numpy(rng.standard_normal((nf, flen)).astype(np.float32)).to(DEV)
            table = torch.tensor([frames.data_ptr() + 4 * flen * f for f in range(nf)], dtype=torch.int64, device=DEV)
            t = torch.linspace(0, 1, flen + 2, dtype=torch.float32)[1:-1]
            weight = (0.5 - (t - 0.5).abs()).to(DEV)
            out = torch.zeros(total, dtype=torch.float32, device=DEV)
            keep += [frames, table, weight]
            outs.append(out)
            d.rows, d.n_frames, d.frame_len, d.stride, d.total, d.weight, d.out = table.data_ptr(), nf, flen, stride, total, weight.data_ptr(), out.data_ptr()
        ws = torch.empty(int(lib.wt_overlap_add_ragged_workspace_bytes(B)), dtype=torch.uint8, device=DEV)
        check(lib.wt_overlap_add_ragged(descs, B, _ptr(ws), _stream(DEV)), "wt_overlap_add_ragged")
        yield f"overlap-add ragged B={B}", sha(*outs)


def ingest_cases():
    B, rates, chans, n_in = 3, (16000, 44100, 24000), (1, 2, 2), (400, 700, 300)
    rng = np.random.default_rng(70)
    for kind in ("fp32", "int16"):
        srcs, descs, n_out = [], (_capi.WtIngestClip * B)(), []
        for d, rate, ch, n in zip(descs, rates, chans, n_in):
            x = rng.standard_normal((ch, n))                                       # planar
            src = torch.from_numpy((x * 8000).astype(np.int16) if kind == "int16" else (0.3 * x).astype(np.float32)).to(DEV)
            srcs.append(src)
            d.src, d.dtype, d.channels, d.n_in, d.ch_stride, d.sample_stride = src.data_ptr(), int(kind == "int16"), ch, n, n, 1
            d.resampler = audio.resampler(rate, 24000, 0)
            d.n_out = int(lib.wt_resampler_out_length(d.resampler, n))
            n_out.append(d.n_out)
        T_pad = max(n_out) + 5
        out = torch.zeros((B, T_pad), dtype=torch.float32, device=DEV)
        ws = torch.empty(int(lib.wt_ingest_workspace_bytes(B)), dtype=torch.uint8, device=DEV)
        check(lib.wt_ingest(descs, B, T_pad, _ptr(out), _ptr(ws), _stream(DEV)), "wt_ingest")
        yield f"ingest {kind} B={B}", sha(out)


def main():
    print("library:", _capi.LIB_PATH, lib.wt_version().decode())
    with torch.cuda.device(0):
        for cases in (mel_cases, stoi_cases, emit_cases, overlap_add_cases, ingest_cases, stft_cases, wavedist_cases):
            try:
                for name, digest in cases():
                    print(f"{name}: sha256 {digest}")
            except _capi.WavTokError as e:
                if cases not in (stft_cases, wavedist_cases):
                    raise
                print(f"({cases.__name__}: {e})")


if __name__ == "__main__":
    main()
