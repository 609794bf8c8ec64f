#!/usr/bin/env python3
"""Loudness in LUFS: what audio.loudness_many costs against the float64 scipy definition per file on the CPU (what callers run
today), the device time of wt_loudness and of each of its launches, what normalize="lufs" adds to a tokenising call against
normalize="rms", and whether the default path moved.
python3 tools/loudness_bench.py [--rounds 5] [--prev tools/lib/libwavtok_hip_prev.so] [--out profiles/loudness_bench.txt]

  (a) audio.loudness_many on clips that lie on the GPU against tests/loudness_ref.py loudness (scipy.signal.lfilter in float64, then
      the gated block mean) per file on clips that lie in host memory: 1 x 3 s, 64 x 3 s, 200 clips of 0.5 - 10 s at five rates and
      one clip of 10 minutes
  (b) the device time of wt_loudness at 64 x 3 s, HIP events around the call, and of each of its four launches (torch.profiler)
  (c) encode_codes_many(normalize="lufs") against encode_codes_many(normalize="rms") of the same build
  (d) the default path, encode_codes_many with no new argument, this build against the parent commit's library
      (tools/build_prev.sh), in child processes alternating prev, new, prev, new (tools/level_bench.py's child)

The method is tools/level_bench.py's: per case the two candidates alternate round by round and each is timed twice per round; the
two series of one candidate are an A/A pair, and the distance of their medians is the spread below which a difference says
nothing.  The CPU side of (a) runs fewer rounds (it takes seconds)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import level_bench as LB  # noqa: E402

SR = LB.SR


def cpu_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-rounds", type=int, default=2)
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--prev", default=os.path.join(ROOT, "tools", "lib", "libwavtok_hip_prev.so"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    res = {"rounds": a.rounds}
    # ---- (d): before this process opens the GPU, so that one process at a time times on it
    log("(d) the default path (no new argument): this build against the parent commit's library, child processes alternating prev, new, prev, new")
    if os.path.exists(a.prev):
        runs = [(tag, LB.run_child(lib, a.rounds, a.files)) for tag, lib in (("prev", a.prev), ("new", ""), ("prev", a.prev), ("new", ""))]
        res["d"] = {}
        for key in [k for k in runs[0][1] if k.startswith("encode") and not k.endswith("_sum")]:
            p, n = [r[key] for t, r in runs if t == "prev"], [r[key] for t, r in runs if t == "new"]
            same = len({r[key + "_sum"] for _t, r in runs}) == 1
            aa = max(abs(p[0] - p[1]), abs(n[0] - n[1]))
            diff = sum(n) / 2 - sum(p) / 2
            log(f"  {key:18s}: prev {p[0]:.4f} {p[1]:.4f} ms, new {n[0]:.4f} {n[1]:.4f} ms, new - prev {diff:+.4f} ms, A/A spread {aa:.4f} ms -> "
                f"{'inside the spread' if abs(diff) <= aa else 'OUTSIDE the spread'}{'' if same else '; OUTPUTS DIFFER'}")
            res["d"][key] = {"prev_ms": [round(v, 4) for v in p], "new_ms": [round(v, 4) for v in n], "aa_spread_ms": round(aa, 4),
                             "new_minus_prev_ms": round(diff, 4), "same_outputs": same}
    else:
        log(f"  not measured: {a.prev} is missing (tools/build_prev.sh builds it)")

    import numpy as np
    import torch
    from tests import loudness_ref as R
    from wavtokenizer_amd import _capi, audio, synth
    m = LB.model()
    res["device"] = torch.cuda.get_device_name(0)
    loads = LB.workloads(a.files)
    long = torch.from_numpy(np.tile(synth.make_clips(1, 60 * SR, seed=77)[0] * np.float32(0.1), 10)).cuda()
    loads["1x600s"] = ([long], [SR], None, 3)

    log(f"(a) audio.loudness_many (clips on the GPU) against scipy lfilter in float64 + gated block mean per file (clips in host memory), {res['device']}")
    res["a"] = {}
    for name, (clips, rates, _codes, inner) in loads.items():
        host = [c.cpu().numpy() for c in clips]
        gpu = lambda: audio.loudness_many(clips, rates)
        cpu = lambda: [R.loudness(x, sr)[0] for x, sr in zip(host, rates)]
        got, want = gpu()[:, 0].cpu().numpy().astype(np.float64), np.array(cpu())
        worst = float(np.abs(got - want)[np.isfinite(want)].max())
        for _ in range(3):
            gpu()
        series = {"gpu": [], "gpu_again": [], "cpu": [], "cpu_again": []}
        for r in range(a.rounds):
            series["gpu"].append(LB.timed(gpu, inner))
            if r < a.cpu_rounds:
                series["cpu"].append(cpu_ms(cpu))
            series["gpu_again"].append(LB.timed(gpu, inner))
            if r < a.cpu_rounds:
                series["cpu_again"].append(cpu_ms(cpu))
        med = {k: float(np.median(v)) for k, v in series.items()}
        for k, v in series.items():
            log(f"  {name} {k:9s}: median {med[k]:10.4f} ms  min {min(v):10.4f}  max {max(v):10.4f}   ({len(v)} rounds)")
        g, c = (med["gpu"] + med["gpu_again"]) / 2, (med["cpu"] + med["cpu_again"]) / 2
        log(f"  {name}: GPU {g:.4f} ms, CPU float64 {c:.2f} ms, CPU / GPU {c / g:.0f}, A/A spread GPU {abs(med['gpu'] - med['gpu_again']):.4f} ms, "
            f"CPU {abs(med['cpu'] - med['cpu_again']):.2f} ms; worst |L_gpu - L_cpu| {worst:.2e} LU over {len(clips)} clips")
        res["a"][name] = {"gpu_ms": round(g, 4), "cpu_ms": round(c, 3), "cpu_over_gpu": round(c / g, 1), "worst_abs_diff_lu": worst}
    del loads["1x600s"]

    log("(b) device time of wt_loudness at 64 x 3 s: HIP events around 20 calls (twice: an A/A pair), then each launch from torch.profiler")
    B, T = 64, 3 * SR
    rows = torch.randn(B, T, device="cuda") * 0.1
    out = torch.empty(B, 3, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    descs = (_capi.WtLoudnessClip * B)()
    for j, d in enumerate(descs):
        d.x, d.n, d.channels, d.channel_stride, d.out, d.blocks = rows[j].data_ptr(), T, 1, 0, out.data_ptr() + 12 * j, None
    ws = torch.empty(int(_capi.lib.wt_loudness_workspace_bytes(B, B * T)), dtype=torch.uint8, device="cuda")
    ws_n = torch.empty(int(_capi.lib.wt_normalize_rows_lufs_workspace_bytes(B, T)), dtype=torch.uint8, device="cuda")
    ws_r = torch.empty(int(_capi.lib.wt_normalize_rows_workspace_bytes(B, T)), dtype=torch.uint8, device="cuda")
    scales = torch.empty(B, device="cuda")
    n = (ctypes.c_int64 * B)(*[T] * B)
    targets = [-23.0, -16.0]

    def normalize_lufs():           # the target alternates: every call's divisor is 10^(+-7 / 20), never 1, so the gain pass always runs
        targets.reverse()
        _capi.check(_capi.lib.wt_normalize_rows_lufs(ptr(rows), B, T, n, SR, targets[0], ptr(scales), ptr(ws_n), stream))

    calls = {"wt_loudness": lambda: _capi.check(_capi.lib.wt_loudness(descs, B, SR, ptr(ws), stream)),
             "wt_normalize_rows_lufs": normalize_lufs,
             "wt_normalize_rows rms": lambda: _capi.check(_capi.lib.wt_normalize_rows(ptr(rows), B, T, n, 1, 1.0, ptr(scales), ptr(ws_r), stream))}
    res["b"] = {}
    for rep in ("first", "again"):
        for name, call in calls.items():
            us = LB.event_ms(call, 20) * 1e3
            res["b"].setdefault(name, {})[rep] = round(us, 2)
            log(f"  {name:24s} {rep:5s}: {us:8.2f} us per call ({B * T * 4 / 1e6:.1f} MB of fp32 samples)")
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(20):
                calls["wt_loudness"]()
            torch.cuda.synchronize()
        seen = 0
        for ev in prof.key_averages():
            if "loud_" in ev.key:
                us = getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)) / max(ev.count, 1)
                short = ev.key.split("(")[0].replace("void wt::", "")[:70]
                log(f"  launch {short:70s}: {us:8.2f} us mean of {ev.count}")
                res["b"].setdefault("launches", {})[short] = round(us, 2)
                seen += 1
        if not seen:
            log("  per launch: not measured (the profiler reported no kernel of wt_loudness)")
    except Exception as e:                                      # noqa: BLE001  (a build of torch without the profiler: say so)
        log(f"  per launch: not measured ({type(e).__name__}: {e})")

    log("(c) encode_codes_many(normalize='lufs') ('new') against encode_codes_many(normalize='rms') ('old', 'composition'), the same build")
    res["c"] = {}
    for name, (clips, rates, _codes, inner) in loads.items():
        new = lambda: m.encode_codes_many(clips, sample_rates=rates, packed=True, normalize="lufs")[0]
        old = lambda: m.encode_codes_many(clips, sample_rates=rates, packed=True, normalize="rms")[0]
        res["c"][name] = LB.pair(name, new, old, a.rounds, inner, True, log)
    m.check_status()
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
