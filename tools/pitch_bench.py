#!/usr/bin/env python3
"""Pitch, periodicity and voiced / unvoiced F1 on the GPU: metrics.periodicity_metrics_many against a torch composition of the same
definition on the GPU, and the device time of the calls.  python3 tools/pitch_bench.py [--rounds 5] [--out profiles/pitch_bench.txt]

Everything warm before anything is timed; a sample is `inner` calls and one stream synchronise; both sides alternate in one
process, and every candidate is timed twice per round: its two series are an A/A pair, and the distance of their medians is the
spread below which a difference says nothing.
  (a) periodicity_metrics_many against the composition a caller could write with torch on the GPU: unfold for the frames, a
      broadcast difference over the 321 lags and 703 terms, cumsum for the running sum, masks and argmax / argmin for the search,
      gather for the parabola, torch.stft for the gate, masked sums for the pair.  The broadcast holds 321 x 703 floats per frame,
      so the composition runs over at most CHUNK frames at a time (a (CHUNK, 321, 703) block: 0.9 GB), clip after clip: 1 x 3 s,
      64 x 3 s pairs, 200 pairs of 0.5 - 10 s, at 16 kHz.  The results are compared.  Peak extra memory of each.
  (b) device time per case, events around the step, through the C ABI on buffers allocated beforehand, queued behind a spinning
      kernel so that the host's launch gaps stay outside, twice (an A/A pair): wt_pitch_pairs, every kernel of the call.  With
      more than 64 pairs the bracket also holds the upload of the descriptors.  --device-only runs (b) alone: under
      `rocprofv3 --kernel-trace --stats -- python3 tools/pitch_bench.py --device-only` the statistics split the step by kernel.
Prints one line per series, one verdict per pair and one JSON line at the end."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from stftd_bench import pair  # noqa: E402

SR, WIN, HOP, TERMS, MAX_LAG, LO, HI = 16000, 1024, 160, 703, 321, 30, 320
CHUNK = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--cases", default="1x3s,64x3s,200x0.5-10s")
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from tests import pitch_ref as R
    from wavtokenizer_amd import metrics
    from wavtokenizer_amd._capi import WtPitchPair, check, lib
    res = {"rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    window = torch.hann_window(WIN, device="cuda")
    a_weight = torch.from_numpy(R.a_weighting64().astype(np.float32)).cuda()
    lag_index = (torch.arange(TERMS, device="cuda")[None, :] + torch.arange(1, MAX_LAG + 1, device="cuda")[:, None])     # [321][703]
    lags = torch.arange(1, MAX_LAG + 1, device="cuda", dtype=torch.float32)
    thr, silence, unvoiced = 0.15, -60.0, 0.5

    def yin(fr):                                                        # (n, 1024) -> f0 (n,), periodicity (n,)
        d = ((fr[:, None, :TERMS] - fr[:, lag_index]) ** 2).sum(-1)    # (n, 321)
        run = d.cumsum(-1)
        dp = torch.where(run > 0, d * lags / run, torch.ones_like(d))
        cur, le, ri = dp[:, LO - 1:HI], dp[:, LO - 2:HI - 1], dp[:, LO:HI + 1]
        ok = (cur < thr) & (cur <= le) & (cur < ri)
        k = torch.where(ok.any(-1), ok.float().argmax(-1), cur.argmin(-1)) + LO - 1            # index into dp: lag - 1
        p, q, r = (dp.gather(1, (k + o)[:, None])[:, 0] for o in (-1, 0, 1))
        den = p - 2 * q + r
        off = torch.where(den > 0, (0.5 * (p - r) / den).clamp(-0.5, 0.5), torch.zeros_like(den))
        return SR / (k + 1 + off), (1 - (q - 0.25 * (p - r) * off)).clamp(0, 1)

    def track(x):                                                       # (T,) -> gated f0 with NaN, gated periodicity
        fr = x.unfold(0, WIN, HOP)
        parts = [yin(fr[i:i + CHUNK]) for i in range(0, fr.shape[0], CHUNK)]
        f0, per = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        Z = torch.stft(x, WIN, HOP, WIN, window=window, center=False, return_complex=True)     # (513, n)
        db = 10 * torch.log10((Z.real ** 2 + Z.imag ** 2).clamp(min=1e-10))
        loud = (torch.maximum(db, db.max() - 80) + a_weight[:, None] - 20).mean(0)
        per = torch.where(loud < silence, torch.zeros_like(per), per)
        return torch.where(per < unvoiced, torch.full_like(f0, float("nan")), f0), per

    def composition(ys, y_hats):
        out = []
        for y, y_hat in zip(ys, y_hats):
            (f0, per), (g0, qer) = track(y), track(y_hat)
            tv, pv = ~torch.isnan(f0), ~torch.isnan(g0)
            both = tv & pv
            cents = 1200 * (torch.log2(f0) - torch.log2(g0))
            tp, fp, fn = both.sum().float(), (~tv & pv).sum().float(), (tv & ~pv).sum().float()
            precision, recall = tp / (tp + fp), tp / (tp + fn)
            out.append(torch.stack([((qer - per) ** 2).mean().sqrt(), (torch.where(both, cents ** 2, torch.zeros_like(cents)).sum() / tp).sqrt(),
                                    2 * precision * recall / (precision + recall)]))
        return torch.stack(out)

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

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    rng = np.random.default_rng(5)
    all_cases = (("1x3s", [3 * SR], 10), ("64x3s", [3 * SR] * 64, 1), ("200x0.5-10s", [int(v) for v in rng.integers(SR // 2, 10 * SR, 200)], 1))
    log(f"(a) periodicity_metrics_many against the torch composition, (b) device time; {res['device']}")
    res["pairs"], res["device_us"] = {}, {}
    for name, lengths, inner in all_cases:
        if name not in a.cases.split(","):
            continue
        ys = [torch.from_numpy(R.recipe(T, 300 + i)).cuda() for i, T in enumerate(lengths)]
        y_hats = [torch.from_numpy(R.decoded(y.cpu().numpy(), (30, 10, 0)[i % 3], i)).cuda() for i, y in enumerate(ys)]
        with torch.inference_mode():
            new, old = (lambda: metrics.periodicity_metrics_many(ys, y_hats)), (lambda: composition(ys, y_hats))
            if a.device_only:
                old = new
            got, want = new().cpu().numpy().astype(np.float64), old().cpu().numpy().astype(np.float64)
            # a frame decided the other way by one of the two fp32 computations moves a pair's numbers: the count of pairs that
            # agree is given beside the largest difference among them
            close = np.array([bool(np.allclose(g, w, rtol=1e-3, atol=1e-4, equal_nan=True)) for g, w in zip(got, want)])
            diff = float(np.nanmax(np.abs(got[close] - want[close]), initial=0.0))
            mem_new, mem_old = peak(new), peak(old)
            res["pairs"][name] = {} if a.device_only else pair("pairs " + name, ("periodicity_metrics_many", "torch composition"), new, old, a.rounds, inner, log)
            res["pairs"][name].update(pairs_in_agreement=int(close.sum()), pairs=len(close), max_abs_diff_of_those=diff,
                                      peak_bytes_new=mem_new, peak_bytes_old=mem_old)
            log(f"  pairs {name}: {int(close.sum())} of {len(close)} pairs agree to 1e-3 relative (the others differ by a frame's decision), largest "
                f"difference among them {diff:.2e}; peak extra memory {mem_new / 2**20:.2f} MiB against {mem_old / 2**20:.2f} MiB")
            # (b) the C ABI on buffers allocated here
            n = len(ys)
            frames = sum(metrics.pitch_frames(T) for T in lengths)
            h = metrics.pitch_handle(0)
            out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            ws = torch.empty(int(lib.wt_pitch_workspace_bytes(n, frames)) // 8 + 1, dtype=torch.int64, device="cuda")
            descs = (WtPitchPair * n)()
            for i in range(n):
                descs[i].reference, descs[i].estimate, descs[i].length, descs[i].out = ys[i].data_ptr(), y_hats[i].data_ptr(), lengths[i], out.data_ptr() + 12 * i
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            call = lambda: check(lib.wt_pitch_pairs(h, descs, n, thr, silence, unvoiced, ctypes.c_void_p(ws.data_ptr()), stream), "wt_pitch_pairs")
            dev = [device_us(call) for _ in range(2)]
            assert np.array_equal(out.cpu().numpy(), new().cpu().numpy(), equal_nan=True)
            res["device_us"][name] = {"wt_pitch_pairs": dev, "frames": 2 * frames}
            log(f"  {name}: device time, events around the step: wt_pitch_pairs ({2 * frames} frames, both signals) {dev[0]:.2f} / {dev[1]:.2f} us, "
                f"{dev[1] * 1e3 / (2 * frames):.2f} ns per frame")
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
