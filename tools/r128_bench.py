#!/usr/bin/env python3
"""The R 128 meter: what audio.true_peak_many and audio.loudness_range_many cost against the float64 scipy / numpy definitions per
file on the CPU (what callers run today) and against a torch composition on the GPU, the device time of the three new C calls
beside the calls they extend, and whether the default path moved.
python3 tools/r128_bench.py [--rounds 5] [--prev tools/lib/libwavtok_hip_prev.so] [--out profiles/r128_bench.txt]

  (a) audio.true_peak_many on clips that lie on the GPU against scipy.signal.upfirdn with the same taps per file, and
      audio.loudness_range_many against tests/r128_ref.py (scipy.signal.lfilter in float64, numpy windows and a sort) per file, on
      clips that lie in host memory: 1 x 3 s, 64 x 3 s, 200 clips of 0.5 - 10 s at five rates
  (b) the same two calls against torch on the GPU: the true peak as one conv1d with the F - 1 phase filters per clip and a max;
      the range as gates, torch.sort and two indices per clip on the short-term series (torch has no recursive filter: the series
      itself is taken from loudness_range_many(series=True), whose time is part of the composition's); 'OUTPUTS DIFFER' there means
      more than 10^-3 dB or LU apart
  (c) device times, HIP events around the call, at 64 x 3 s: wt_true_peak beside wt_level (which reads the same bytes: the floor),
      wt_loudness_range beside wt_loudness, wt_normalize_rows_lufs_tp beside wt_normalize_rows_lufs
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
    from scipy.signal import upfirdn
    from tests import r128_ref as Q
    from wavtokenizer_amd import _capi, audio
    res["device"] = torch.cuda.get_device_name(0)
    loads = LB.workloads(a.files)

    def series_of(gpu, cpu, inner):
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
        return series, {k: float(np.median(v)) for k, v in series.items()}

    log(f"(a) clips on the GPU against the float64 definitions per file on clips in host memory, {res['device']}")
    res["a"] = {}
    for name, (clips, rates, _codes, inner) in loads.items():
        host = [c.cpu().numpy() for c in clips]

        def cpu_peak():
            return [float(np.abs(upfirdn(Q.taps(Q.factor(sr)).astype(np.float64), x.astype(np.float64), Q.factor(sr))).max()) for x, sr in zip(host, rates)]

        def cpu_range():
            return [Q.loudness_range(Q.short_term(x, sr)[0])[0] for x, sr in zip(host, rates)]

        for what, gpu, cpu, column in (("true_peak_many", lambda: audio.true_peak_many(clips, rates), cpu_peak, 0),
                                       ("loudness_range_many", lambda: audio.loudness_range_many(clips, rates), cpu_range, 3)):
            got = gpu()[:, column].cpu().numpy().astype(np.float64)
            want = np.array(cpu())
            if what == "true_peak_many":
                want = 20.0 * np.log10(want)
            ok = np.isfinite(want)
            worst = float(np.abs(got - want)[ok].max()) if ok.any() else 0.0
            series, med = series_of(gpu, cpu, inner)
            for k, v in series.items():
                log(f"  {name} {what} {k:9s}: median {med[k]:10.4f} ms  min {min(v):10.4f}  max {max(v):10.4f}   ({len(v)} rounds)")
            g, c = (med["gpu"] + med["gpu_again"]) / 2, (med["cpu"] + med["cpu_again"]) / 2
            log(f"  {name} {what}: GPU {g:.4f} ms, CPU float64 {c:.2f} ms, CPU / GPU {c / g:.0f}, A/A spread GPU {abs(med['gpu'] - med['gpu_again']):.4f} ms, "
                f"CPU {abs(med['cpu'] - med['cpu_again']):.2f} ms; worst |gpu - cpu| {worst:.2e} {'dB' if column == 0 else 'LU'} over {int(ok.sum())} of {len(clips)} clips")
            res["a"][name + " " + what] = {"gpu_ms": round(g, 4), "cpu_ms": round(c, 3), "cpu_over_gpu": round(c / g, 1), "worst_abs_diff": worst}

    log("(b) the same calls ('new') against a torch composition on the GPU ('old', 'composition')")
    res["b"] = {}
    phase = {F: torch.from_numpy(np.stack([Q.taps(F)[p:48:F][::-1].copy() for p in range(1, F)])).cuda()[:, None, :] for F in (4, 2)}

    def torch_peak(clips, rates):
        out = []
        for x, sr in zip(clips, rates):
            F = Q.factor(sr)
            y = torch.nn.functional.conv1d(x[None, None], phase[F], padding=24 // F)
            out.append(torch.maximum(y.abs().max(), x.abs().max()))
        return 20.0 * torch.log10(torch.stack(out))

    def torch_range(clips, rates):
        _out, _mom, sht = audio.loudness_range_many(clips, rates, series=True)
        out = []
        for s in sht:
            z = torch.pow(10.0, (s.double() + 0.691) / 10.0)
            keep = s > -70.0
            if not bool(keep.any()):
                out.append(torch.tensor(float("nan"), device=s.device))
                continue
            rel = -0.691 + 10.0 * torch.log10(z[keep].mean()) - 20.0
            kept = torch.sort(s[keep & (s > rel)]).values
            m = kept.shape[0]
            out.append(kept[(19 * (m - 1) + 10) // 20] - kept[((m - 1) + 5) // 10])
        return torch.stack(out)

    def close(x, y, tol):            # (the compositions round elsewhere: agreement within tol, NaN where both have none)
        x, y = x.double().cpu(), y.double().cpu()
        return bool(((x - y).abs() <= tol).logical_or(x.isnan() & y.isnan()).logical_or(x == y).all())

    for name, (clips, rates, _codes, inner) in loads.items():
        same = close(audio.true_peak_many(clips, rates)[:, 0], torch_peak(clips, rates), 1e-3)
        res["b"][name + " true_peak_many"] = LB.pair(name + " true_peak", lambda: audio.true_peak_many(clips, rates), lambda: torch_peak(clips, rates),
                                                     a.rounds, inner, same, log)
        same = close(audio.loudness_range_many(clips, rates)[:, 3], torch_range(clips, rates), 1e-3)
        res["b"][name + " loudness_range_many"] = LB.pair(name + " range", lambda: audio.loudness_range_many(clips, rates),
                                                          lambda: torch_range(clips, rates), a.rounds, inner, same, log)

    log("(c) device time at 64 x 3 s: HIP events around 20 calls (twice: an A/A pair)")
    B, T = 64, 3 * SR
    rows = torch.randn(B, T, device="cuda") * 0.1
    out = torch.empty(B, 9, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    lv, ld, tp, lr = (_capi.WtLevelClip * B)(), (_capi.WtLoudnessClip * B)(), (_capi.WtTruePeakClip * B)(), (_capi.WtLoudnessRangeClip * B)()
    for j in range(B):
        lv[j].x, lv[j].n, lv[j].out = rows[j].data_ptr(), T, out.data_ptr() + 36 * j
        for d in (ld[j], tp[j], lr[j]):
            d.x, d.n, d.channels, d.channel_stride, d.out = rows[j].data_ptr(), T, 1, 0, out.data_ptr() + 36 * j
    lib = _capi.lib
    ws = torch.empty(max(int(lib.wt_level_workspace_bytes(B, B * T)), int(lib.wt_true_peak_workspace_bytes(B, B * T)),
                         int(lib.wt_loudness_range_workspace_bytes(B, B * T)), int(lib.wt_normalize_rows_lufs_tp_workspace_bytes(B, T))),
                     dtype=torch.uint8, device="cuda")
    scales = torch.empty(B, device="cuda")
    n = (ctypes.c_int64 * B)(*[T] * B)
    targets = [-23.0, -16.0]

    def normalize(tp_ceiling):      # the target alternates: every call's divisor is 10^(+-7 / 20), never 1, so the gain pass always runs
        targets.reverse()
        if tp_ceiling is None:
            _capi.check(lib.wt_normalize_rows_lufs(ptr(rows), B, T, n, SR, targets[0], ptr(scales), ptr(ws), stream))
        else:
            _capi.check(lib.wt_normalize_rows_lufs_tp(ptr(rows), B, T, n, SR, targets[0], tp_ceiling, ptr(scales), ptr(ws), stream))

    calls = {"wt_level": lambda: _capi.check(lib.wt_level(lv, B, ptr(ws), stream)),
             "wt_true_peak": lambda: _capi.check(lib.wt_true_peak(tp, B, SR, ptr(ws), stream)),
             "wt_loudness": lambda: _capi.check(lib.wt_loudness(ld, B, SR, ptr(ws), stream)),
             "wt_loudness_range": lambda: _capi.check(lib.wt_loudness_range(lr, B, SR, ptr(ws), stream)),
             "wt_normalize_rows_lufs": lambda: normalize(None),
             "wt_normalize_rows_lufs_tp": lambda: normalize(-1.0)}
    res["c"] = {}
    for rep in ("first", "again"):
        for name, call in calls.items():
            us = LB.event_ms(call, 20) * 1e3
            res["c"].setdefault(name, {})[rep] = round(us, 2)
            log(f"  {name:26s} {rep:5s}: {us:8.2f} us per call ({B * T * 4 / 1e6:.1f} MB of fp32 samples)")
    for new, old in (("wt_true_peak", "wt_level"), ("wt_loudness_range", "wt_loudness"), ("wt_normalize_rows_lufs_tp", "wt_normalize_rows_lufs")):
        mean = lambda k: (res["c"][k]["first"] + res["c"][k]["again"]) / 2
        log(f"  {new} / {old}: {mean(new) / mean(old):.3f}")
        res["c"][new + " / " + old] = round(mean(new) / mean(old), 3)
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
