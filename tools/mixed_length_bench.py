#!/usr/bin/env python3
"""Tokenising a dataset of clips of different lengths: the reference's infer.py loop (one encode_infer call per file) against
WavTokenizer.encode_infer_many, encode only.  python3 tools/mixed_length_bench.py [--arch hop600] [--files 200] [--min-s 0.5]
[--max-s 20] [--seed 0]

One seeded set of file lengths.  Each method runs on a fresh model twice: "cold" is the first pass over the dataset (every plan,
graph and workspace is created on the way, as a one-off tokenising job pays), "warm" the second pass over the same files.
Reported per method and pass: files/s, audio-s/s, plans created; for encode_infer_many also the padding overhead of its calls
(padded samples / real samples - 1).  Both methods are checked to return the same codes.  Prints one JSON line at the end.

--decode [--files 64 --min-s 1 --max-s 10 --rounds 5]: the way back.  Features of random codes for the same kind of length set;
the loop of one decode call per clip (what a caller without decode_many writes) against WavTokenizer.decode_many, on one model
with every plan warm: the two methods alternate `rounds` times in the same process, and the medians, the spread (min .. max) of
each and the ratio of the medians are reported.  Both methods are checked to return the same waveforms."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("WAVTOK_MAX_PLANS", "4096")          # count plans, do not evict them
from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth  # noqa: E402
from wavtokenizer_amd.mixed_length import group_clips  # noqa: E402

SR = 24000


def fresh_model(arch, sd):
    m = WavTokenizer.from_arch(arch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    m = m.eval().cuda()
    m._ensure_engine()
    created = [0]
    plan = m._engine.plan

    def counting_plan(kind, B, length, flags, device, sites=0):
        if m._engine._key(kind, B, length, flags, device, sites) not in m._engine.plans:
            created[0] += 1
        return plan(kind, B, length, flags, device, sites)
    m._engine.plan = counting_plan
    return m, created


def run(method, m, wavs):
    bw = torch.tensor([0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if method == "loop":
        out = [m.encode_infer(w[None], bandwidth_id=bw) for w in wavs]
    else:
        out = m.encode_infer_many(wavs, bandwidth_id=bw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main_decode(a):
    from wavtokenizer_amd.mixed_length import group_frames
    arch = NAMED_ARCHS[a.arch]
    rng = np.random.default_rng(a.seed)
    frames = [arch.frames(int(x)) for x in rng.integers(int(a.min_s * SR), int(a.max_s * SR) + 1, size=a.files)]
    m, created = fresh_model(arch, synth.make_state_dict(arch, seed=0))
    feats = [m.codes_to_features(torch.from_numpy(rng.integers(0, arch.vq_bins, size=(1, 1, L))).cuda())[0].contiguous() for L in frames]
    bw = torch.tensor([0])
    groups = group_frames(frames)
    methods = {"loop": lambda: [m.decode(f[None], bandwidth_id=bw) for f in feats],
               "many": lambda: m.decode_many(feats, bandwidth_id=bw)}
    outs, times = {}, {"loop": [], "many": []}
    for name, fn in methods.items():          # every plan (and graph) is created and recorded before anything is timed
        for _ in range(3):
            outs[name] = fn()
        torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in methods.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    m.check_status()
    same = all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(outs["loop"], outs["many"]))
    res = {"mode": "decode", "arch": a.arch, "clips": a.files, "frames_total": sum(frames), "rounds": a.rounds,
           "many_calls": len(groups), "many_padding_overhead": round(sum(L_pad * len(idx) for L_pad, idx in groups) / sum(frames) - 1, 4),
           "plans_created": created[0], "identical_outputs": same}
    for name, t in times.items():
        res[f"{name}_ms"] = [round(x, 3) for x in t]
        res[f"{name}_median_ms"] = round(float(np.median(t)), 3)
        res[f"{name}_spread_ms"] = round(max(t) - min(t), 3)
        print(f"{name:4s}: median {np.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  ({a.files} clips, {sum(frames)} frames)", flush=True)
    res["speedup"] = round(res["loop_median_ms"] / res["many_median_ms"], 2)
    print(json.dumps(res), flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="hop600", choices=sorted(NAMED_ARCHS))
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--max-s", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--decode", action="store_true", help="time decode_many against the loop of one decode call per clip")
    ap.add_argument("--rounds", type=int, default=5, help="--decode: alternations of the two methods")
    a = ap.parse_args()
    if a.decode:
        return main_decode(a)
    arch = NAMED_ARCHS[a.arch]
    rng = np.random.default_rng(a.seed)
    lengths = [int(x) for x in rng.integers(int(a.min_s * SR), int(a.max_s * SR) + 1, size=a.files)]
    wavs = [torch.from_numpy(synth.make_clips(1, T, seed=a.seed * 100003 + i)[0]).cuda() for i, T in enumerate(lengths)]
    audio_s = sum(lengths) / SR
    sd = synth.make_state_dict(arch, seed=0)
    groups, solo = group_clips(lengths, arch.hop)
    padded = sum(T_pad * len(idx) for T_pad, idx in groups) + sum(lengths[i] for i in solo)
    res = {"arch": a.arch, "files": a.files, "audio_s": round(audio_s, 1), "distinct_lengths": len(set(lengths)),
           "many_calls": len(groups) + len(solo), "many_padding_overhead": round(padded / sum(lengths) - 1, 4)}
    outs = {}
    for method in ("loop", "many"):
        m, created = fresh_model(arch, sd)
        for pas in ("cold", "warm"):
            before = created[0]
            dt, out = run(method, m, wavs)
            res[f"{method}_{pas}_files_per_s"] = round(a.files / dt, 2)
            res[f"{method}_{pas}_audio_s_per_s"] = round(audio_s / dt, 1)
            res[f"{method}_{pas}_plans_created"] = created[0] - before
            print(f"{method:4s} {pas}: {dt:8.3f} s  {a.files / dt:9.2f} files/s  {audio_s / dt:10.1f} audio-s/s  "
                  f"{created[0] - before} plans created", flush=True)
        m.check_status()
        outs[method] = out
        del m
        torch.cuda.empty_cache()
    bad = [i for i, ((f1, c1), (f2, c2)) in enumerate(zip(outs["loop"], outs["many"]))
           if f1.shape != f2.shape or not (torch.equal(c1, c2) and torch.equal(f1, f2))]
    same = not bad
    res["identical_outputs"] = same
    for i in bad[:10]:
        (f1, c1), (f2, c2) = outs["loop"][i], outs["many"][i]
        if f1.shape != f2.shape:
            print(f"clip {i} ({lengths[i]} samples): shapes {tuple(f1.shape)} vs {tuple(f2.shape)}", flush=True)
            continue
        nc = int((c1 != c2).sum())
        print(f"clip {i} ({lengths[i]} samples, {c1.shape[-1]} frames): {nc} codes differ, first at frame "
              f"{int((c1 != c2).reshape(-1).nonzero()[0]) if nc else -1}; features differ at "
              f"{int((f1 != f2).any(1).sum())} frames", flush=True)
    for pas in ("cold", "warm"):
        res[f"speedup_{pas}"] = round(res[f"many_{pas}_files_per_s"] / res[f"loop_{pas}_files_per_s"], 2)
    print(json.dumps(res), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
