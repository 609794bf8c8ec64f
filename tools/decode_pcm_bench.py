#!/usr/bin/env python3
"""Synthesising to PCM: WavTokenizer.decode_pcm / decode_pcm_many against the composition they replace, decode_codes /
decode_codes_many finished by hand (audio.convert_audio per clip and rate, stereo expand and interleave, audio.to_pcm16, copy to
the host).  python3 tools/decode_pcm_bench.py [--arch hop600] [--rounds 7] [--seed 0] [--out profiles/decode_pcm_bench.txt]

One process, one model, every plan and graph warm before anything is timed.  Four cases:
  (a) B = 1 x 3 s, int16 at 24 kHz, graph replay        decode_pcm          vs  decode_codes, to_pcm16
  (b) 64 x 3 s, int16 at 24 kHz, on the GPU             decode_pcm          vs  decode_codes, to_pcm16
  (c) 64 x 3 s, int16 at 24 kHz, into pinned host memory
                                                        decode_pcm_many     vs  decode_codes, to_pcm16, one copy, one wait
  (d) 200 clips of 0.5 - 10 s to rates drawn from 16 000 / 22 050 / 24 000 / 44 100 / 48 000, every second one stereo
      interleaved, int16, to the host                   decode_pcm_many     vs  decode_codes_many; then per clip convert_audio,
                                                                                expand + interleave, to_pcm16, copy to the host
Per case the two candidates alternate round by round, and each is timed TWICE per round (new, old, new, old): the two series
of one candidate are an A/A pair, and the distance of their medians is the spread below which a difference between the
candidates says nothing.  A sample is `inner` calls and one stream synchronise.  Both sides run with set_strict_status(False)
and set_check_codes("off"), so that a sample holds launches and no per-call synchronise but the ones the case itself asks for (the
wait behind a copy to the host).  Both candidates are checked to return the same samples.  Prints one line per series, one verdict
per case, files/s and audio-s/s for (d), and one JSON line at the end."""
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
    m.set_check_codes("off")
    rng = np.random.default_rng(a.seed)
    bw = torch.tensor([0])
    res = {"arch": a.arch, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    log(f"synthesising to PCM against the composition over decode_codes: {a.arch}, {res['device']}, {a.rounds} rounds")
    L3 = 3 * SR // arch.hop_length
    draw = lambda B, L: torch.from_numpy(rng.integers(0, arch.vq_bins, size=(1, B, L))).cuda()

    for case, B, inner in (("a", 1, 50), ("b", 64, 10)):
        codes = draw(B, L3)
        new = lambda: m.decode_pcm(codes, bandwidth_id=bw)
        old = lambda: audio.to_pcm16(m.decode_codes(codes, bandwidth_id=bw), limit=0.99)[:, None]
        log(f"({case}) B = {B} x 3 s, int16 at 24 kHz on the GPU{', graph replay' if B <= m._graph_max_clips else ''}")
        res[case] = compare(case, new, old, a.rounds, inner, torch.equal(new(), old()), log)

    codes = draw(64, L3)
    rows = [codes[:, j] for j in range(64)]
    pin = torch.empty((64, m._wave_len(L3)), dtype=torch.int16, pin_memory=True)

    def old_c():
        pin.copy_(audio.to_pcm16(m.decode_codes(codes, bandwidth_id=bw), limit=0.99), non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return pin

    new = lambda: m.decode_pcm_many(rows, packed=True, device="cpu", bandwidth_id=bw)[0]
    log(f"(c) 64 x 3 s, int16 at 24 kHz, into pinned host memory ({pin.numel() * 2} bytes)")
    res["c"] = compare("c", new, old_c, a.rounds, 10, torch.equal(new(), old_c().reshape(-1)), log)

    clips, rates, stereo = [], [], []
    for i in range(a.files):
        sr = int(rng.choice(RATES))
        L = max(1, int(round(rng.uniform(0.5, 10.0) * SR / arch.hop_length)))
        clips.append(draw(1, L)[:, 0])
        rates.append(sr)
        stereo.append(bool(i % 2))
    seconds = sum(m._wave_len(int(c.shape[1])) / SR for c in clips)

    def by_hand():
        out = []
        for w, sr, st in zip(m.decode_codes_many(clips, bandwidth_id=bw), rates, stereo):
            r = audio.convert_audio(w[:, None], SR, sr, 1)[0] if sr != SR else w
            if st:
                r = r.expand(2, -1).t()                      # (n, 2): to_pcm16 makes it contiguous, i.e. interleaves
            out.append(audio.to_pcm16(r, limit=0.99).cpu())
        return out

    chans = [2 if st else 1 for st in stereo]
    new_d = lambda: m.decode_pcm_many(clips, sample_rates=rates, channels=chans, channels_last=True, device="cpu", bandwidth_id=bw)

    log(f"(d) {a.files} clips of 0.5 - 10 s ({seconds:.1f} s of audio) to five rates, every second one stereo interleaved, int16, to the host")
    same = all(x.shape == y.reshape(x.shape[0], -1).shape and torch.equal(x.reshape(-1), y.reshape(-1)) for x, y in zip(new_d(), by_hand()))
    res["d"] = compare("d", new_d, by_hand, a.rounds, 1, same, log)
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
