#!/usr/bin/env python3
"""Tokenising from PCM: WavTokenizer.encode_codes / encode_codes_many against the composition they replace, encode_infer /
encode_infer_many fed by hand (upload, / 32768, audio.convert_audio per file), codes taken.  python3 tools/encode_codes_bench.py
[--arch hop600] [--rounds 7] [--seed 0] [--out profiles/encode_codes_bench.txt]

One process, one model, every plan and graph warm before anything is timed.  Four cases:
  (a) B = 1 x 3 s, fp32 on the GPU, graph replay        encode_codes        vs  encode_infer
  (b) 64 x 3 s, fp32 on the GPU                         encode_codes        vs  encode_infer
  (c) 64 x 3 s int16 in pinned host memory              encode_codes_many   vs  upload, / 32768, encode_infer
  (d) 200 host clips of 0.5 - 10 s, int16, rates drawn from 16 000 / 22 050 / 24 000 / 44 100 / 48 000, half of them stereo
      interleaved (pageable memory, as a file reader leaves them)
                                                        encode_codes_many   vs  per file upload, / 32768, convert_audio; then
                                                                                encode_infer_many, codes taken
Per case the two candidates alternate round by round, and each is timed TWICE per round (new, old, new, old): the two series
of one candidate are an A/A pair, and the distance of their medians is the spread below which a difference between the
candidates says nothing.  A sample is `inner` calls and one stream synchronise.  Both sides run with set_strict_status(False),
so that a sample holds launches and no per-call synchronise.  Both candidates are checked to return the same codes.  Prints one
line per series, one verdict per case, files/s and audio-s/s for (d), and one JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, audio, synth  # noqa: E402

SR = 24000
RATES = [16000, 22050, 24000, 44100, 48000]


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def compare(name, new, old, rounds, inner, same, log):
    """Alternates new / old / new / old per round; returns the case's record."""
    for fn in (new, old):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    series = {"new": [], "old": [], "new_again": [], "old_again": []}
    for _ in range(rounds):
        for key, fn in (("new", new), ("old", old), ("new_again", new), ("old_again", old)):
            series[key].append(timed(fn, inner))
    med = {k: float(np.median(v)) for k, v in series.items()}
    for k, v in series.items():
        log(f"  {name} {k:9s}: median {med[k]:9.4f} ms  min {min(v):9.4f}  max {max(v):9.4f}   ({rounds} rounds x {inner} calls)")
    new_ms, old_ms = (med["new"] + med["new_again"]) / 2, (med["old"] + med["old_again"]) / 2
    aa = max(abs(med["new"] - med["new_again"]), abs(med["old"] - med["old_again"]))
    slower = new_ms - old_ms > aa
    log(f"  {name}: new {new_ms:.4f} ms, old {old_ms:.4f} ms, old / new {old_ms / new_ms:.3f}, difference {old_ms - new_ms:+.4f} ms, "
        f"A/A spread {aa:.4f} ms -> {'SLOWER than the composition by more than the spread' if slower else 'not slower than the composition'}"
        f"{'' if same else '; OUTPUTS DIFFER'}")
    return {"new_ms": round(new_ms, 4), "old_ms": round(old_ms, 4), "aa_spread_ms": round(aa, 4), "old_over_new": round(old_ms / new_ms, 3),
            "slower_beyond_spread": bool(slower), "identical_outputs": bool(same),
            "medians_ms": {k: round(v, 4) for k, v in med.items()}}


def pcm16(x):
    return torch.from_numpy(np.rint(x * np.float32(0.9 * 32768.0)).astype(np.int16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="hop600", choices=sorted(NAMED_ARCHS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--files", type=int, default=200, help="clips of case (d)")
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
    rng = np.random.default_rng(a.seed)
    bw = torch.tensor([0])
    res = {"arch": a.arch, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    log(f"tokenising from PCM against the composition over encode_infer: {a.arch}, {res['device']}, {a.rounds} rounds")

    for case, B, inner in (("a", 1, 50), ("b", 64, 10)):
        wav = torch.from_numpy(synth.make_clips(B, 3 * SR, seed=10 + B)).cuda()
        new = lambda: m.encode_codes(wav, bandwidth_id=bw)
        old = lambda: m.encode_infer(wav, bandwidth_id=bw)[1]
        log(f"({case}) B = {B} x 3 s, fp32 on the GPU{', graph replay' if B <= m._graph_max_clips else ''}")
        res[case] = compare(case, new, old, a.rounds, inner, torch.equal(new(), old()), log)

    host = pcm16(synth.make_clips(64, 3 * SR, seed=5)).pin_memory()
    rows = list(host)
    new = lambda: m.encode_codes_many(rows, packed=True, bandwidth_id=bw)[0]
    old = lambda: m.encode_infer(host.cuda(non_blocking=True).float() / 32768, bandwidth_id=bw)[1]
    log(f"(c) 64 x 3 s int16 in pinned host memory ({host.numel() * 2} bytes)")
    res["c"] = compare("c", new, old, a.rounds, 10, torch.equal(new(), old().reshape(-1)), log)

    clips, rates = [], []
    for i in range(a.files):
        sr = int(rng.choice(RATES))
        n = int(sr * rng.uniform(0.5, 10.0))
        x = pcm16(synth.make_clips(2 if i % 2 else 1, n, seed=1000 + i, sample_rate=sr))
        clips.append(x.t().contiguous() if i % 2 else x[0].clone())         # (T, 2) interleaved, or (T,)
        rates.append(sr)
    seconds = sum(c.shape[0] / sr for c, sr in zip(clips, rates))

    def by_hand():
        wavs = []
        for c, sr in zip(clips, rates):
            x = c.cuda().float() / 32768
            x = x.t() if x.dim() == 2 else x[None]
            wavs.append(audio.convert_audio(x[None], sr, SR)[0, 0])
        return [codes for _f, codes in m.encode_infer_many(wavs, bandwidth_id=bw)]

    new = lambda: m.encode_codes_many(clips, sample_rates=rates, channels_last=True, bandwidth_id=bw)
    log(f"(d) {a.files} host clips of 0.5 - 10 s ({seconds:.1f} s of audio), int16, five rates, every second one stereo interleaved")
    same = all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(new(), by_hand()))
    res["d"] = compare("d", new, by_hand, a.rounds, 1, same, log)
    for side in ("new", "old"):
        ms = res["d"][side + "_ms"]
        res["d"][side + "_files_per_s"] = round(a.files / ms * 1e3, 1)
        res["d"][side + "_audio_s_per_s"] = round(seconds / ms * 1e3, 1)
        log(f"  d {side}: {res['d'][side + '_files_per_s']:.1f} files/s, {res['d'][side + '_audio_s_per_s']:.1f} audio-s/s")

    m.check_status()
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(v["identical_outputs"] for v in res.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
