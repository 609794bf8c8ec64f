#!/usr/bin/env python3
"""Residual VQ tokenising: what encode_codes(n_q=None) costs now, what encode_codes(n_q=3) costs against what a caller could write
before, and the device time of one round.  python3 tools/rvq_bench.py [--rounds 7] [--prev tools/lib/libwavtok_hip_prev.so]
[--out profiles/rvq_bench.txt]

Three-codebook hop-600 model on synthetic weights; every plan and graph warm before anything is timed; a sample is `inner`
calls and one stream synchronise; both sides of a pair alternate, and every candidate is timed twice per round: its two series
are an A/A pair, and the distance of their medians is the spread below which a difference says nothing.
  (a) encode_codes(n_q=None), this build against the parent commit's library (tools/build_prev.sh), 64 x 3 s and B = 1 under graph
      replay.  A library is bound when the package is imported, so each side is a child process of its own (--child), and the
      children alternate prev, new, prev, new as tools/ab_lib.sh alternates them: the two runs of one library are the A/A pair.
      Expected: a difference inside the spread (the call takes the plan, the launches and the recording it took before).
  (b) encode_codes(n_q=3) against feature_extractor.encodec.encoder(x) followed by three rounds of torch matmul / max /
      embedding / subtract on the GPU, 64 x 3 s and 32 x 30 s.  Timing only: the torch rounds decide near ties in their own way.
  (c) device time of vq_residual_kernel and of one vq.argmin round at 64 x 3 s, from wt_plan_set_timing / wt_plan_read_timing
      (events around the step; each bracket adds a few microseconds, as profiles/r04_kernel_stats.md notes for the tool).
Prints one line per series, one verdict per pair and one JSON line at the end."""
import argparse
import ctypes
import dataclasses
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 24000


def timed(fn, inner):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def model(n_q=3):
    import torch
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth
    arch = dataclasses.replace(NAMED_ARCHS["hop600"], num_quantizers=n_q)
    m = WavTokenizer.from_arch(arch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, seed=0).items()}, strict=False)
    m = m.eval().cuda()
    m.set_strict_status(False)
    return m


def clips(B, seconds, seed):
    import torch
    from wavtokenizer_amd import synth
    return torch.from_numpy(synth.make_clips(B, seconds * SR, seed=seed)).cuda()


def child(rounds):
    """(a), one library: medians of encode_codes(n_q=None) at 64 x 3 s and at B = 1 under graph replay, as one JSON line."""
    import numpy as np
    import torch
    m = model()
    out = {}
    for name, B, inner in (("64x3s", 64, 10), ("1x3s_graph", 1, 50)):
        wav = clips(B, 3, seed=10 + B)
        fn = lambda: m.encode_codes(wav)
        for _ in range(5):
            fn()
        out[name] = float(np.median([timed(fn, inner) for _ in range(rounds)]))
        out[name + "_sum"] = int(fn().sum())
    m.check_status()
    print("CHILD " + json.dumps(out), flush=True)


def run_child(lib, rounds):
    env = dict(os.environ)
    if lib:
        env["WAVTOK_HIP_LIB"] = lib
    else:
        env.pop("WAVTOK_HIP_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(rounds)], env=env, capture_output=True,
                       text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")]
    if p.returncode or not line:
        raise RuntimeError(f"child with {lib or 'this build'} failed ({p.returncode}): {p.stderr[-600:]}")
    return json.loads(line[-1][6:])


def pair(name, new, old, rounds, inner, log):
    import numpy as np
    for fn in (new, old):
        for _ in range(3):
            fn()
    series = {"new": [], "old": [], "new_again": [], "old_again": []}
    for _ in range(rounds):
        for key, fn in (("new", new), ("old", old), ("new_again", new), ("old_again", old)):
            series[key].append(timed(fn, inner))
    med = {k: float(np.median(v)) for k, v in series.items()}
    for k, v in series.items():
        log(f"  {name} {k:9s}: median {med[k]:9.4f} ms  min {min(v):9.4f}  max {max(v):9.4f}   ({rounds} rounds x {inner} calls)")
    new_ms, old_ms = (med["new"] + med["new_again"]) / 2, (med["old"] + med["old_again"]) / 2
    aa = max(abs(med["new"] - med["new_again"]), abs(med["old"] - med["old_again"]))
    log(f"  {name}: encode_codes(n_q=3) {new_ms:.4f} ms, encoder + torch rounds {old_ms:.4f} ms, old / new {old_ms / new_ms:.3f}, A/A spread {aa:.4f} ms")
    return {"new_ms": round(new_ms, 4), "old_ms": round(old_ms, 4), "aa_spread_ms": round(aa, 4), "old_over_new": round(old_ms / new_ms, 3)}


def step_time(m, plan, filt, call, calls):
    """Mean device time per timed step whose name contains filt, over `calls` direct calls: (ms per step, steps per call)."""
    from wavtokenizer_amd._capi import check, lib
    import torch
    check(lib.wt_plan_set_timing(plan, filt.encode()), "wt_plan_set_timing")
    ms, n = ctypes.c_double(), ctypes.c_int64()
    check(lib.wt_plan_read_timing(plan, ctypes.byref(ms), ctypes.byref(n), 1), "wt_plan_read_timing")
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    check(lib.wt_plan_read_timing(plan, ctypes.byref(ms), ctypes.byref(n), 1), "wt_plan_read_timing")
    check(lib.wt_plan_set_timing(plan, None), "wt_plan_set_timing")
    return ms.value / max(n.value, 1), n.value / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--prev", default=os.path.join(ROOT, "tools", "lib", "libwavtok_hip_prev.so"))
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.rounds)
        return 0
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    res = {"rounds": a.rounds}
    # ---- (a): before this process opens the GPU, so that one process at a time times on it
    log("(a) encode_codes(n_q=None): this build against the parent commit's library, child processes alternating prev, new, prev, new")
    if os.path.exists(a.prev):
        runs = [(tag, run_child(lib, a.rounds)) for tag, lib in (("prev", a.prev), ("new", ""), ("prev", a.prev), ("new", ""))]
        res["a"] = {}
        for shape in ("64x3s", "1x3s_graph"):
            p, n = [r[shape] for t, r in runs if t == "prev"], [r[shape] for t, r in runs if t == "new"]
            same = len({r[shape + "_sum"] for _t, r in runs}) == 1
            aa = max(abs(p[0] - p[1]), abs(n[0] - n[1]))
            diff = sum(n) / 2 - sum(p) / 2
            log(f"  {shape:11s}: prev {p[0]:.4f} {p[1]:.4f} ms, new {n[0]:.4f} {n[1]:.4f} ms, new - prev {diff:+.4f} ms, A/A spread {aa:.4f} ms -> "
                f"{'inside the spread' if abs(diff) <= aa else 'OUTSIDE the spread'}{'' if same else '; CODES DIFFER'}")
            res["a"][shape] = {"prev_ms": [round(v, 4) for v in p], "new_ms": [round(v, 4) for v in n], "aa_spread_ms": round(aa, 4),
                               "new_minus_prev_ms": round(diff, 4), "same_codes": same}
    else:
        log(f"  not measured: {a.prev} is missing (tools/build_prev.sh builds it)")

    import torch
    import torch.nn.functional as F
    from wavtokenizer_amd import _capi
    m = model()
    res["device"] = torch.cuda.get_device_name(0)
    sd = m.state_dict()
    books = [sd["feature_extractor.encodec.quantizer.vq.layers.%d._codebook.embed" % k].cuda() for k in range(3)]
    ees = [e.pow(2).sum(1)[None] for e in books]
    enc = m.feature_extractor.encodec.encoder

    def by_hand(wav):
        r = enc(wav[:, None, :]).transpose(1, 2).reshape(-1, 512)
        out = []
        for e, ee in zip(books, ees):
            c = (-(r.pow(2).sum(1, keepdim=True) - 2 * r @ e.t() + ee)).max(dim=-1).indices
            out.append(c)
            r = r - F.embedding(c, e)
        return torch.stack(out)

    # ---- (b)
    log(f"(b) encode_codes(n_q=3) against encoder(x) + three torch rounds (matmul / max / embedding / subtract), {res['device']}")
    res["b"] = {}
    for name, B, sec, inner in (("64x3s", 64, 3, 10), ("32x30s", 32, 30, 3)):
        wav = clips(B, sec, seed=20 + B)
        with torch.inference_mode():
            new, old = (lambda: m.encode_codes(wav, n_q=3)), (lambda: by_hand(wav))
            agree = float((new().reshape(3, -1) == old()).float().mean())
            res["b"][name] = pair(name, new, old, a.rounds, inner, log)
        res["b"][name]["codes_in_agreement"] = round(agree, 5)
        log(f"  {name}: {agree:.3%} of the codes agree (near ties decided differently, and every later round of such a frame)")

    # ---- (c)
    log("(c) device time per step at 64 x 3 s (events around the step, direct launches)")
    wav = clips(64, 3, seed=84)
    m.encode_codes(wav, n_q=3)
    (key, (plan, _ws)), = [(k, v) for k, v in m._engine.plans.items()
                           if k[0] == _capi.WT_PLAN_ENCODE and k[3] & _capi.WT_PLAN_FLAG_RVQ and k[1] == 64 and k[2] == 3 * SR]
    call = lambda: m.encode_codes(wav, n_q=3)
    res["c"] = {}
    for rep in ("first", "again"):               # the same measurement twice: its own A/A pair
        for filt in ("vq.residual", "vq.argmin"):
            ms, per_call = step_time(m, plan, filt, call, 20)
            res["c"].setdefault(filt, {})[rep] = round(ms * 1e3, 2)
            log(f"  {filt:12s} {rep:5s}: {ms * 1e3:8.2f} us per step ({per_call:.0f} timed steps per call)")
    m.check_status()
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
