#!/usr/bin/env python3
"""Long recordings in segments: WavTokenizer.encode_codes_segmented(_many) / decode_pcm_segmented(_many) against what a caller could
write before them: audio.convert_audio once and a loop of encode_codes per segment; a loop of decode_codes per segment, then
audio.linear_overlap_add, audio.convert_audio and audio.to_pcm16.
python3 tools/segmented_bench.py [--arch hop600] [--rounds 3] [--seed 0] [--out profiles/segmented_bench.txt]

One process, one model, every plan and graph warm before anything is timed.  Cases:
  (a) one 10-minute recording, 24 kHz fp32 on the GPU, 10 s segments at the reference's default 1 % overlap (stride 237 600);
      tokenising and synthesis (int16 at 24 kHz on the GPU) timed separately
  (b) the same recording in 1 s segments at 1 % overlap (the encodec_48khz setting, encoder/model.py:296)
  (c) 20 recordings of 30 s to 5 min at five rates, int16 from the host, 10 s segments; synthesis to the host at the recording's
      own rate, every second recording stereo interleaved; files/s and audio-s/s
  (d) the uniform batches of (a) on the plain encode plan against the mixed-length plan (the shipped default is named)
and the device time of wt_overlap_add_ragged alone on (a)'s geometry with the bytes it moves.
Per case the two candidates alternate round by round, each timed TWICE per round (new, old, new, old): the two series of one
candidate are an A/A pair, and the distance of their medians is the spread below which a difference says nothing.  Both sides
run with set_strict_status(False) and set_check_codes("off").  Both candidates are checked to return the same codes / samples."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, _capi, audio, synth  # noqa: E402
from wavtokenizer_amd.segmented import segment_plan  # noqa: E402

SR = 24000
RATES = [16000, 22050, 24000, 44100, 48000]
HBM_PEAK_GBS = 8000.0        # MI355X: 8 TB/s


def timed(fn, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def compare(name, new, old, rounds, same, log, labels=("new", "old")):
    """Alternates new / old / new / old per round; returns the case's record."""
    for fn in (new, old):
        fn()
    torch.cuda.synchronize()
    series = {"new": [], "old": [], "new_again": [], "old_again": []}
    for _ in range(rounds):
        for key, fn in (("new", new), ("old", old), ("new_again", new), ("old_again", old)):
            series[key].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in series.items()}
    for k, v in series.items():
        log(f"  {name} {k.replace('new', labels[0]).replace('old', labels[1]):14s}: median {med[k]:10.3f} ms  min {min(v):10.3f}  max {max(v):10.3f}   ({rounds} rounds)")
    new_ms, old_ms = (med["new"] + med["new_again"]) / 2, (med["old"] + med["old_again"]) / 2
    aa = max(abs(med["new"] - med["new_again"]), abs(med["old"] - med["old_again"]))
    slower = new_ms - old_ms > aa
    log(f"  {name}: {labels[0]} {new_ms:.3f} ms, {labels[1]} {old_ms:.3f} ms, {labels[1]} / {labels[0]} {old_ms / new_ms:.3f}, A/A spread {aa:.3f} ms -> "
        f"{labels[0]} is {'SLOWER by more than the spread' if slower else 'not slower'}{'' if same else '; OUTPUTS DIFFER'}")
    return {"new_ms": round(new_ms, 3), "old_ms": round(old_ms, 3), "aa_spread_ms": round(aa, 3), "old_over_new": round(old_ms / new_ms, 3),
            "slower_beyond_spread": bool(slower), "identical_outputs": bool(same), "medians_ms": {k: round(v, 3) for k, v in med.items()}}


def encode_loop(m, W, S, stride):
    """What a caller writes today: W (1, T) at the codec rate -> the codes of every segment."""
    offs, lens = segment_plan(int(W.shape[-1]), S, stride)
    return [m.encode_codes(W[:, o:o + n]) for o, n in zip(offs, lens)]


def synth_loop(m, sc, bw):
    """decode_codes per segment, then the cross-fade: (1, length) fp32 at the codec rate."""
    _offs, lens = segment_plan(sc.length, sc.segment_length, sc.stride)
    dec = [m.decode_codes(c, bandwidth_id=bw)[..., :n] for c, n in zip(sc.segments(), lens)]
    return audio.linear_overlap_add(dec, sc.stride)[..., :sc.length]


def ola_device_time(S, stride, total, log):
    """wt_overlap_add_ragged alone on one recording's geometry, rows at a pitch of S + 600 as a decode batch leaves them."""
    offs, lens = segment_plan(total, S, stride)
    pitch = S + 600
    arena = torch.randn(len(offs) * pitch, device="cuda")
    table = torch.tensor([arena.data_ptr() + 4 * i * pitch for i in range(len(offs))], dtype=torch.int64).cuda()
    t = torch.linspace(0, 1, min(S, total) + 2, dtype=torch.float32)[1:-1]
    w = (0.5 - (t - 0.5).abs()).cuda()
    out = torch.empty(total, device="cuda")
    d = (_capi.WtOverlapAddClip * 1)()
    d[0].rows, d[0].n_frames, d[0].frame_len, d[0].stride, d[0].total = table.data_ptr(), len(offs), min(S, total), stride, total
    d[0].weight, d[0].out = w.data_ptr(), out.data_ptr()
    ws = torch.empty(64, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: _capi.check(_capi.lib.wt_overlap_add_ragged(d, 1, ctypes.c_void_p(ws.data_ptr()), stream), "wt_overlap_add_ragged")
    for _ in range(5):
        call()
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    moved = 4 * (sum(lens) + total)                          # every frame sample read once, every output written once (the triangle stays in cache)
    gbs = moved / med / 1e6
    log(f"wt_overlap_add_ragged alone, {len(offs)} frames of {S} at stride {stride}, {total} samples: median {med * 1e3:.1f} us of 20 (event "
        f"timing, launch included), {moved / 1e6:.1f} MB moved, {gbs:.0f} GB/s = {100 * gbs / HBM_PEAK_GBS:.1f} % of the {HBM_PEAK_GBS / 1e3:.0f} TB/s HBM peak")
    return {"median_us": round(med * 1e3, 1), "bytes": moved, "gb_per_s": round(gbs, 1), "fraction_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="hop600", choices=sorted(NAMED_ARCHS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--minutes", type=float, default=10.0, help="length of the recording of (a), (b), (d)")
    ap.add_argument("--files", type=int, default=20, help="recordings of case (c)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    arch = NAMED_ARCHS[a.arch]
    m = WavTokenizer.from_arch(arch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, seed=0).items()}, strict=False)
    m = m.eval().cuda()
    m.set_strict_status(False)
    m.set_check_codes("off")
    rng = np.random.default_rng(a.seed)
    bw = torch.tensor([0])
    res = {"arch": a.arch, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    log(f"long recordings in segments against the per-segment loops: {a.arch}, {res['device']}, {a.rounds} rounds")
    T = int(a.minutes * 60 * SR)
    # a long recording: a few seconds of the synthetic clip, tiled and modulated so that no two segments are equal
    base = synth.make_clips(1, 10 * SR, seed=5)[0]
    long_wav = np.tile(base, -(-T // base.size))[:T] * (0.6 + 0.4 * np.sin(np.arange(T) * (2 * np.pi / (7.3 * SR)))).astype(np.float32)
    wav = torch.from_numpy(long_wav.astype(np.float32)).cuda()

    def same_codes(sc, want):
        return sc.n_segments == len(want) and all(torch.equal(g, w) for g, w in zip(sc.segments(), want))

    for case, S in (("a", 10 * SR), ("b", SR)):
        stride = max(1, int(0.99 * S))
        n_seg = len(segment_plan(T, S, stride)[0])
        log(f"({case}) one recording of {a.minutes:g} min, 24 kHz fp32 on the GPU, segments of {S} at stride {stride}: {n_seg} segments")
        new_e = lambda: m.encode_codes_segmented(wav, S, stride)
        old_e = lambda: encode_loop(m, audio.convert_audio(wav[None, None], SR, SR, 1)[0], S, stride)
        res[case + "_encode"] = compare(case + " encode", new_e, old_e, a.rounds, same_codes(new_e(), old_e()), log)
        sc = new_e()
        new_s = lambda: m.decode_pcm_segmented(sc, bandwidth_id=bw)
        old_s = lambda: audio.to_pcm16(audio.convert_audio(synth_loop(m, sc, bw)[:, None], SR, SR, 1)[0], limit=0.99)
        res[case + "_synth"] = compare(case + " synth", new_s, old_s, a.rounds, torch.equal(new_s(), old_s()), log)
        for k in ("_encode", "_synth"):
            res[case + k]["audio_s_per_s"] = round(T / SR / res[case + k]["new_ms"] * 1e3, 1)
            log(f"  {case}{k}: {res[case + k]['audio_s_per_s']:.1f} audio-s/s through the new call")

    S, stride = 10 * SR, int(0.99 * 10 * SR)
    log(f"(d) the uniform batches of (a): the plain encode plan ('new', the shipped default) against the mixed-length plan ('old')")

    def mixed_form():
        m._segment_uniform_mixed = True
        try:
            return m.encode_codes_segmented(wav, S, stride)
        finally:
            m._segment_uniform_mixed = False

    plain_form = lambda: m.encode_codes_segmented(wav, S, stride)
    res["d"] = compare("d", plain_form, mixed_form, a.rounds, torch.equal(plain_form().codes, mixed_form().codes), log, labels=("plain", "mixed"))

    clips, rates, secs = [], [], []
    for i in range(a.files):
        sr = RATES[i % len(RATES)]
        sec = float(rng.uniform(30.0, 300.0))
        n = int(sec * sr)
        x = np.tile(base, -(-int(sec * SR) // base.size))[:int(sec * SR)]
        idx = np.minimum((np.arange(n) * (SR / sr)).astype(np.int64), x.size - 1)      # (a crude rate change: the content does not matter)
        clips.append(torch.from_numpy(np.rint(x[idx] * 32767.0 * (0.5 + 0.5 * rng.random())).astype(np.int16)))
        rates.append(sr)
        secs.append(sec)
    seconds = sum(secs)
    chans = [1 + i % 2 for i in range(a.files)]
    log(f"(c) {a.files} recordings of 30 s - 5 min ({seconds:.0f} s of audio) at five rates, int16 from the host, segments of {S} at stride {stride}")
    new_e = lambda: m.encode_codes_segmented_many(clips, S, stride, sample_rates=rates)
    old_e = lambda: [encode_loop(m, audio.convert_audio((c.cuda().float() / 32768.0)[None, None], sr, SR, 1)[0], S, stride) for c, sr in zip(clips, rates)]
    res["c_encode"] = compare("c encode", new_e, old_e, a.rounds, all(same_codes(g, w) for g, w in zip(new_e(), old_e())), log)
    segs = new_e()
    new_s = lambda: m.decode_pcm_segmented_many(segs, sample_rates=rates, channels=chans, channels_last=True, device="cpu", bandwidth_id=bw)

    def old_s():
        out = []
        for sc, sr, ch in zip(segs, rates, chans):
            r = audio.convert_audio(synth_loop(m, sc, bw)[:, None], SR, sr, 1)[0]
            if ch == 2:
                r = r.expand(2, -1).t()                      # (n, 2): to_pcm16 makes it contiguous, i.e. interleaves
            out.append(audio.to_pcm16(r, limit=0.99).cpu())
        return out

    same = all(torch.equal(x.reshape(-1), y.reshape(-1)) for x, y in zip(new_s(), old_s()))
    res["c_synth"] = compare("c synth", new_s, old_s, a.rounds, same, log)
    for k in ("c_encode", "c_synth"):
        for side in ("new", "old"):
            ms = res[k][side + "_ms"]
            res[k][side + "_files_per_s"] = round(a.files / ms * 1e3, 2)
            res[k][side + "_audio_s_per_s"] = round(seconds / ms * 1e3, 1)
            log(f"  {k} {side}: {res[k][side + '_files_per_s']:.2f} files/s, {res[k][side + '_audio_s_per_s']:.1f} audio-s/s")

    res["overlap_add_ragged"] = ola_device_time(10 * SR, int(0.99 * 10 * SR), T, log)
    m.check_status()
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(v.get("identical_outputs", True) for v in res.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
