#!/usr/bin/env python3
"""The mel distance on the GPU: metrics.mel_distance_many against the torch composition a caller could write before, and the
device time of the frame kernel.  python3 tools/mel_bench.py [--rounds 7] [--out profiles/mel_bench.txt]

Everything warm before anything is timed; a sample is `inner` calls and one stream synchronise; both sides of a pair alternate in
one process, and every candidate is timed twice per round: its two series are an A/A pair, and the distance of their medians is
the spread below which a difference says nothing.
  (a) mel_distance_many against torch.stft -> abs -> filterbank matmul -> clamp -> log -> mean of |.| on the GPU (the filterbank
      is wt_mel_tables', so both sides compute one definition), with a Python loop over the clips where the lengths differ:
      1 x 3 s, 64 x 3 s pairs, 200 pairs of 0.5 - 10 s.  The two results are compared (largest difference of a clip's distance).
      Where the lengths are equal the composition holds its two (B, T) batches before the timed region, as a caller with
      batched tensors would: no torch.stack is timed or counted in its peak memory.
  (b) device time per case, events around the step, through the C ABI on buffers allocated beforehand (no allocator work in the
      bracket), queued behind a spinning kernel so that the host's launch gaps stay outside, each twice (its own A/A pair):
      the frame kernel alone (wt_mel_spectrogram, log, on one signal) and the wt_mel_distance call (the frame kernel on both
      signals plus the per-clip sum).  With more than 64 clips both brackets also hold the upload of the descriptors.
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
    log(f"  {name}: mel_distance_many {new_ms:.4f} ms, torch composition {old_ms:.4f} ms, old / new {old_ms / new_ms:.3f}, A/A spread {aa:.4f} ms")
    return {"new_ms": round(new_ms, 4), "old_ms": round(old_ms, 4), "aa_spread_ms": round(aa, 4), "old_over_new": round(old_ms / new_ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from wavtokenizer_amd import metrics
    from wavtokenizer_amd._capi import WtMelClip, check, lib
    res = {"rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    fb_host = np.zeros((513, 100), np.float32)
    assert lib.wt_mel_tables(SR, 1024, 100, None, fb_host.ctypes.data_as(ctypes.c_void_p)) == 0
    fb = torch.from_numpy(fb_host).cuda().t().contiguous()              # [100][513]
    window = torch.hann_window(1024, device="cuda")

    def logmel(x):                                                      # (B, T) -> (B, 100, F)
        S = torch.stft(x, 1024, 256, window=window, center=True, pad_mode="reflect", return_complex=True).abs()
        return torch.log(torch.clamp(fb @ S, min=1e-7))

    def composition(y_hats, ys):
        if isinstance(ys, torch.Tensor):                                # equal lengths: (B, T) batches
            return (logmel(y_hats) - logmel(ys)).abs().mean(dim=(1, 2))
        return torch.stack([(logmel(p[None]) - logmel(q[None])).abs().mean() for p, q in zip(y_hats, ys)])

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
    cases = (("1x3s", [3 * SR], 50), ("64x3s", [3 * SR] * 64, 10), ("200x0.5-10s", [int(v) for v in rng.integers(SR // 2, 10 * SR, 200)], 3))
    log(f"(a) mel_distance_many against the torch composition, {res['device']}")
    res["a"], res["b"] = {}, {}
    for name, lengths, inner in cases:
        ys = [torch.from_numpy((0.1 * rng.standard_normal(T)).astype(np.float32)).cuda() for T in lengths]
        y_hats = [y + 0.01 * torch.randn_like(y) for y in ys]
        batched = len(set(lengths)) == 1
        cy_hats, cys = (torch.stack(y_hats), torch.stack(ys)) if batched else (y_hats, ys)
        with torch.inference_mode():
            new, old = (lambda: metrics.mel_distance_many(y_hats, ys)), (lambda: composition(cy_hats, cys))
            diff = float((new() - old()).abs().max())
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            new()
            mem_new = torch.cuda.max_memory_allocated() - base
            torch.cuda.reset_peak_memory_stats()
            old()
            mem_old = torch.cuda.max_memory_allocated() - base
            res["a"][name] = pair(name, new, old, a.rounds, inner, log)
            res["a"][name].update(max_abs_diff=diff, peak_bytes_new=int(mem_new), peak_bytes_old=int(mem_old))
            log(f"  {name}: largest difference of a clip's distance {diff:.2e}; peak extra memory {mem_new / 2**20:.2f} MiB against {mem_old / 2**20:.2f} MiB")
            # (b) the C ABI on buffers allocated here
            n = len(ys)
            F = [1 + T // 256 for T in lengths]
            frames = sum(F)
            h = metrics.mel_handle(SR, 1024, 256, 100, 0)
            spec = torch.empty(100 * frames, dtype=torch.float32, device="cuda")
            dist = torch.empty(n, dtype=torch.float32, device="cuda")
            ws = torch.empty(int(lib.wt_mel_workspace_bytes(n, frames)) // 8 + 1, dtype=torch.int64, device="cuda")
            d_spec, d_dist = (WtMelClip * n)(), (WtMelClip * n)()
            off = 0
            for i in range(n):
                d_spec[i].a, d_spec[i].length, d_spec[i].out = ys[i].data_ptr(), lengths[i], spec.data_ptr() + 4 * off
                d_dist[i].a, d_dist[i].b, d_dist[i].length, d_dist[i].out = y_hats[i].data_ptr(), ys[i].data_ptr(), lengths[i], dist.data_ptr() + 4 * i
                off += 100 * F[i]
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            wsp = ctypes.c_void_p(ws.data_ptr())
            frame_call = lambda: check(lib.wt_mel_spectrogram(h, d_spec, n, 1, wsp, stream), "wt_mel_spectrogram")
            dist_call = lambda: check(lib.wt_mel_distance(h, d_dist, n, wsp, stream), "wt_mel_distance")
            dev = {"frame_kernel": [device_us(frame_call) for _ in range(2)], "distance_call": [device_us(dist_call) for _ in range(2)]}
            assert torch.equal(dist, new())
            res["b"][name] = dict(dev, frames=frames)
            log(f"  {name}: device time, events around the step: frame kernel on one signal ({frames} frames) {dev['frame_kernel'][0]:.2f} / "
                f"{dev['frame_kernel'][1]:.2f} us, {dev['frame_kernel'][1] * 1e3 / frames:.2f} ns per frame; wt_mel_distance (both signals and the "
                f"per-clip sum) {dev['distance_call'][0]:.2f} / {dev['distance_call'][1]:.2f} us")
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
