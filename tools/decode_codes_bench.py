#!/usr/bin/env python3
"""Decoding from codes: WavTokenizer.decode_codes / decode_codes_many against the composition they replace,
decode(codes_to_features(codes)) / decode_many fed from codes_to_features.  python3 tools/decode_codes_bench.py [--arch hop600]
[--rounds 7] [--seed 0] [--out profiles/decode_codes_bench.txt]

One process, one model, every plan and graph warm before anything is timed.  Four cases:
  (a) B = 1, L = 120 frames, graph replay          decode_codes            vs  decode(codes_to_features(.))
  (b) B = 64, L = 120                              decode_codes            vs  decode(codes_to_features(.))
  (c) B = 64, L = 120, inputs in pinned host memory: codes uploaded + decode_codes  vs  features uploaded + decode
  (d) 64 clips of 1 - 10 s                         decode_codes_many       vs  decode_many(codes_to_features per clip)
Per case the two candidates alternate round by round, and each is timed TWICE per round (new, old, new, old): the two series
of one candidate are an A/A pair, and the distance of their medians is the spread below which a difference between the
candidates says nothing.  A sample is `inner` calls and one stream synchronise.  The model runs with set_check_codes("off") and
set_strict_status(False), so that a sample holds launches and no per-call synchronise (with the defaults both candidates wait
for the GPU after every small call, the composition twice); cases (a) and (b) are then repeated with the defaults
(set_check_codes("sync"), automatic strict status: "a-default", "b-default"), what a caller who changes nothing pays: there
decode_codes waits for the whole decode before it looks at the bad-index word, while the composition waits for the gather
alone.  Both candidates are checked to return the same waveforms.  Prints
one line per series, one verdict per case and one JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth  # noqa: E402

SR = 24000


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
    m.set_check_codes("off")
    m.set_strict_status(False)
    rng = np.random.default_rng(a.seed)
    bw = torch.tensor([0])
    res = {"arch": a.arch, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    log(f"decode from codes against decode(codes_to_features(codes)): {a.arch}, {res['device']}, {a.rounds} rounds")

    def codes_of(B, L):
        return torch.from_numpy(rng.integers(0, arch.vq_bins, size=(1, B, L)))

    def pair(c):
        return (lambda: m.decode_codes(c, bandwidth_id=bw)), (lambda: m.decode(m.codes_to_features(c), bandwidth_id=bw))

    for case, B, inner in (("a", 1, 50), ("b", 64, 10)):
        c = codes_of(B, 120).cuda()
        new, old = pair(c)
        log(f"({case}) B = {B}, L = 120{', graph replay' if B <= m._graph_max_clips else ''}")
        res[case] = compare(case, new, old, a.rounds, inner, torch.equal(new(), old()), log)

    m.set_check_codes("sync")
    m.set_strict_status(None)
    for case, B, inner in (("a-default", 1, 50), ("b-default", 64, 10)):
        c = codes_of(B, 120).cuda()
        new, old = pair(c)
        log(f"({case}) B = {B}, L = 120, set_check_codes(\"sync\") and automatic strict status (the defaults)")
        res[case] = compare(case, new, old, a.rounds, inner, torch.equal(new(), old()), log)
    m.set_check_codes("off")
    m.set_strict_status(False)

    c_host = codes_of(64, 120).pin_memory()
    f_host = m.codes_to_features(c_host.cuda()).cpu().pin_memory()
    new = lambda: m.decode_codes(c_host.cuda(non_blocking=True), bandwidth_id=bw)
    old = lambda: m.decode(f_host.cuda(non_blocking=True), bandwidth_id=bw)
    log(f"(c) B = 64, L = 120, inputs in pinned host memory: {c_host.numel() * 8} bytes of codes, {f_host.numel() * 4} bytes of features")
    res["c"] = compare("c", new, old, a.rounds, 10, torch.equal(new(), old()), log)

    frames = [arch.frames(int(x)) for x in rng.integers(1 * SR, 10 * SR + 1, size=64)]
    clips = [torch.from_numpy(rng.integers(0, arch.vq_bins, size=(1, L))).cuda() for L in frames]
    new = lambda: m.decode_codes_many(clips, bandwidth_id=bw)
    old = lambda: m.decode_many([m.codes_to_features(c)[0] for c in clips], bandwidth_id=bw)
    log(f"(d) 64 clips of 1 - 10 s ({sum(frames)} frames)")
    same = all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(new(), old()))
    res["d"] = compare("d", new, old, a.rounds, 1, same, log)

    m.check_status()
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(v["identical_outputs"] for v in res.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
