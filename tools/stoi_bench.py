#!/usr/bin/env python3
"""STOI on the GPU: metrics.stoi_many against what a caller could do before, and the device time of the call.
python3 tools/stoi_bench.py [--rounds 5] [--kernel-stats CSV] [--out profiles/stoi_bench.txt]

Three cases at 24 kHz: 1 x 3 s, 64 x 3 s pairs, 200 pairs of 0.5 - 10 s.  Everything warm before anything is timed; a sample is
`inner` calls and one stream synchronise; both sides of a pair alternate in one process, and every candidate is timed twice per
round: its two series are an A/A pair, and the distance of their medians is the spread below which a difference says nothing.
  (a) stoi_many against a vectorised torch composition of the same definition on the GPU (zero-stuffing and conv1d for the
      resampler, unfold for the frames, boolean indexing for the kept frames, which waits for the host, torch.fft.rfft, a matmul
      for the bands), a Python loop over the pairs.  The two results are compared.
  (b) stoi_many against the float64 numpy definition (tests/stoi_ref.py) on the CPU, the copy of the pair to the host included:
      two passes (an A/A pair) of one call each; for the 200 pairs every tenth pair is run and the time is given per pair.
  (c) device time of the wt_stoi call, STOI and ESTOI, events around the step, through the C ABI on buffers allocated beforehand,
      queued behind a spinning kernel so that the host's launch gaps stay outside, each twice (its own A/A pair).  The call
      launches its six kernels itself, so events cannot bracket one of them.
  (d) the device time per kernel, from a kernel trace: `--calls-only 64x3s` is the program to put under the profiler's kernel
      trace with statistics, and `--kernel-stats <its *_kernel_stats.csv>` makes this run read that file and write the split
      (below the JSON line, and into the JSON line as "d").  Without the argument the section is left out and a line says so.
Prints one line per series, one verdict per pair and one JSON line at the end."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 24000
EPS = 2.0 ** -52


def timed(fn, inner):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def pair(name, new, old, rounds, inner, log):
    import numpy as np
    for fn in (new, old):
        for _ in range(2):
            fn()
    series = {"new": [], "old": [], "new_again": [], "old_again": []}
    for _ in range(rounds):
        for key, fn in (("new", new), ("old", old), ("new_again", new), ("old_again", old)):
            series[key].append(timed(fn, inner))
    med = {k: float(np.median(v)) for k, v in series.items()}
    for k, v in series.items():
        log(f"  {name} {k:9s}: median {med[k]:10.4f} ms  min {min(v):10.4f}  max {max(v):10.4f}   ({rounds} rounds x {inner} calls)")
    new_ms, old_ms = (med["new"] + med["new_again"]) / 2, (med["old"] + med["old_again"]) / 2
    aa = max(abs(med["new"] - med["new_again"]), abs(med["old"] - med["old_again"]))
    log(f"  {name}: stoi_many {new_ms:.4f} ms, torch composition {old_ms:.4f} ms, old / new {old_ms / new_ms:.3f}, A/A spread {aa:.4f} ms")
    return {"new_ms": round(new_ms, 4), "old_ms": round(old_ms, 4), "aa_spread_ms": round(aa, 4), "old_over_new": round(old_ms / new_ms, 3)}


def kernel_split(path, calls, log):
    """The stoi_* rows of a profiler's kernel statistics CSV (Name, Calls, TotalDurationNs, AverageNs, MinNs, MaxNs)."""
    import csv
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "stoi_" in r["Name"]]
    if not rows:
        raise SystemExit(f"{path} holds no stoi_* kernel")
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {}
    log(f"(d) kernel trace of {calls} stoi_many calls on the 64 x 3 s pairs (half STOI, half ESTOI; --calls-only 64x3s): device time per kernel")
    for r in rows:
        name = r["Name"].split("wt::")[1].split("<")[0]
        out[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                     "max_us": round(float(r["MaxNs"]) / 1e3, 2), "share": round(float(r["TotalDurationNs"]) / tot, 4)}
        k = out[name]
        log(f"  {name:26s} calls {k['calls']:3d}  average {k['avg_us']:8.2f} us  min {k['min_us']:8.2f}  max {k['max_us']:8.2f}  "
            f"{100 * k['share']:5.1f} % of the call's kernels")
    log(f"  the call's kernels together: {tot / calls / 1e3:.2f} us per call")
    return out


TRACED_CALLS = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--calls-only", default="", metavar="CASE",
                    help="only run stoi_many on this case ten times as STOI and ten times as ESTOI: the program to put under a kernel trace")
    ap.add_argument("--kernel-stats", default="", metavar="CSV", help="the *_kernel_stats.csv of a kernel trace of --calls-only 64x3s: section (d)")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from tests import stoi_ref as R
    from wavtokenizer_amd import metrics
    from wavtokenizer_amd._capi import WtStoiClip, check, lib
    res = {"rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    h64, p, q, L = R.resample_filter(SR)
    taps = torch.from_numpy(h64[::-1].copy().astype(np.float32)).cuda()[None, None]
    win = torch.from_numpy(R.window64().astype(np.float32)).cuda()
    bands = torch.zeros(15, 257, device="cuda")
    for b, (lo, hi) in enumerate(R.BAND_EDGES):
        bands[b, lo:hi] = 1.0

    def resample(v):
        up = torch.zeros(v.shape[0] * p, device="cuda")
        up[::p] = v
        up = torch.nn.functional.pad(up, (L, L + q))
        return torch.nn.functional.conv1d(up[None, None], taps, stride=q)[0, 0][: -(-v.shape[0] * p // q)]

    def rownorm(t, dim):
        t = t - t.mean(dim=dim, keepdim=True)
        return t / (t.norm(dim=dim, keepdim=True) + EPS)

    def composition_one(x, y, ext):
        x, y = resample(x), resample(y)
        K0 = -(-(x.shape[0] - 256) // 128)
        xf, yf = x.unfold(0, 256, 128)[:K0] * win, y.unfold(0, 256, 128)[:K0] * win
        norms = xf.norm(dim=1)
        keep = norms + EPS > 0.01 * (norms.max() + EPS)
        tob = []
        for f in (xf[keep], yf[keep]):
            K = f.shape[0]
            rebuilt = torch.zeros(K + 1, 128, device="cuda")
            rebuilt[:K] += f[:, :128]
            rebuilt[1:] += f[:, 128:]
            fr = rebuilt.view(-1).unfold(0, 256, 128)[: K - 1] * win
            tob.append(torch.sqrt(torch.fft.rfft(fr, n=512, dim=1).abs().square() @ bands.t()))          # [J][15]
        if tob[0].shape[0] < 30:
            return torch.full((), 1e-5, device="cuda")
        X, Y = (t.unfold(0, 30, 1) for t in tob)                                                         # [S][15][30]
        if ext:
            xn, yn = rownorm(rownorm(X, 2), 1), rownorm(rownorm(Y, 2), 1)
            return (xn * yn).sum() / (30 * X.shape[0])
        alpha = X.norm(dim=2, keepdim=True) / (Y.norm(dim=2, keepdim=True) + EPS)
        Yp = torch.minimum(alpha * Y, X * (1 + 10 ** (15 / 20)))
        return (rownorm(X, 2) * rownorm(Yp, 2)).sum() / (15 * X.shape[0])

    def composition(xs, ys, ext=False):
        return torch.stack([composition_one(x, y, ext) for x, y in zip(xs, ys)])

    def device_us(call):
        """Median device time of call() over 20 brackets, in microseconds."""
        ts = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(2_000_000)                                # the host queues the launches while the device spins
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return round(float(np.median(ts)), 2)

    rng = np.random.default_rng(5)
    cases = (("1x3s", [3 * SR], 20, 1), ("64x3s", [3 * SR] * 64, 3, 1), ("200x0.5-10s", [int(v) for v in rng.integers(SR // 2, 10 * SR, 200)], 1, 10))
    log(f"stoi_many at 24 kHz, {res['device']}")
    res["a"], res["b"], res["c"] = {}, {}, {}
    for name, lengths, inner, cpu_step in cases:
        if a.calls_only and a.calls_only != name:
            continue
        xs_host = [R.speechlike(T, SR, seed=i) for i, T in enumerate(lengths)]
        ys_host = [R.noisy(x, (20, 0, -10)[i % 3], seed=i) for i, x in enumerate(xs_host)]
        xs, ys = [torch.from_numpy(x).cuda() for x in xs_host], [torch.from_numpy(y).cuda() for y in ys_host]
        n = len(xs)
        if a.calls_only:
            for ext in (False, True):
                for _ in range(TRACED_CALLS // 2):
                    metrics.stoi_many(xs, ys, sample_rate=SR, extended=ext)
            torch.cuda.synchronize()
            return 0
        with torch.inference_mode():
            new, old = (lambda: metrics.stoi_many(xs, ys, sample_rate=SR)), (lambda: composition(xs, ys))
            diff = float((new() - old()).abs().max())
            diff_e = float((metrics.stoi_many(xs, ys, sample_rate=SR, extended=True) - composition(xs, ys, True)).abs().max())
            log(f"(a) {name}: against the torch composition; largest difference of a pair's STOI {diff:.2e}, ESTOI {diff_e:.2e}")
            res["a"][name] = pair(name, new, old, a.rounds, inner, log)
            res["a"][name].update(max_abs_diff=diff, max_abs_diff_extended=diff_e)
            # (b) float64 numpy on the CPU, the copies to the host included
            sel = list(range(0, n, cpu_step))
            cpu = []
            for _ in range(2):
                t0 = time.perf_counter()
                d64 = [R.stoi64(xs[i].cpu().numpy(), ys[i].cpu().numpy(), SR) for i in sel]
                cpu.append((time.perf_counter() - t0) * 1e3 / len(sel))
            gpu = new()
            diff64 = max(abs(float(gpu[i]) - d) for i, d in zip(sel, d64))
            new_ms = res["a"][name]["new_ms"]
            res["b"][name] = {"cpu_ms_per_pair": [round(c, 2) for c in cpu], "pairs_run": len(sel), "gpu_ms_per_pair": round(new_ms / n, 5),
                              "max_abs_diff": diff64}
            log(f"(b) {name}: float64 numpy on the CPU, {len(sel)} of the {n} pairs, two passes: {cpu[0]:.2f} / {cpu[1]:.2f} ms per pair; "
                f"stoi_many {new_ms / n:.5f} ms per pair ({new_ms:.4f} ms for the {n}); largest difference {diff64:.2e}")
            # (c) the C ABI on buffers allocated here
            h = metrics.stoi_handle(SR, 0)
            sizes = [metrics.stoi_frames(T, SR) for T in lengths]
            out = torch.empty(n, dtype=torch.float32, device="cuda")
            ws = torch.empty(int(lib.wt_stoi_workspace_bytes(h, n, sum(s[0] for s in sizes), sum(s[1] for s in sizes))) // 8 + 1,
                             dtype=torch.int64, device="cuda")
            descs = (WtStoiClip * n)()
            for i in range(n):
                descs[i].clean, descs[i].processed, descs[i].length, descs[i].out = xs[i].data_ptr(), ys[i].data_ptr(), lengths[i], out.data_ptr() + 4 * i
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            wsp = ctypes.c_void_p(ws.data_ptr())
            dev = {}
            for key, ext in (("stoi", 0), ("estoi", 1)):
                call = lambda: check(lib.wt_stoi(h, descs, n, ext, wsp, stream, None), "wt_stoi")
                dev[key] = [device_us(call) for _ in range(2)]
                if not ext:
                    assert torch.equal(out, gpu)
            frames = sum(s[1] for s in sizes)
            res["c"][name] = dict(dev, candidate_frames=frames, resampled_samples=sum(s[0] for s in sizes))
            log(f"(c) {name}: device time of wt_stoi, events around the step ({frames} candidate frames): STOI {dev['stoi'][0]:.2f} / "
                f"{dev['stoi'][1]:.2f} us, ESTOI {dev['estoi'][0]:.2f} / {dev['estoi'][1]:.2f} us")
    split = []
    if a.kernel_stats:
        res["d"] = kernel_split(a.kernel_stats, TRACED_CALLS, split.append)
    log(json.dumps(res))
    for line in split or ["(d) no --kernel-stats file was given: the device time per kernel is left out of this run"]:
        log(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
