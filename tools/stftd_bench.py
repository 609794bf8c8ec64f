#!/usr/bin/env python3
"""The STFT distance, SI-SDR and SNR on the GPU: metrics.stft_distance_many and the pair si_sdr_many + snr_many against the torch
compositions a caller could write before, the device time of the calls, and round_trip_report against the five separate round
trips.  python3 tools/stftd_bench.py [--rounds 7] [--out profiles/stftd_bench.txt]

Everything warm before anything is timed; a sample is `inner` calls and one stream synchronise; both sides of a pair alternate in
one process, and every candidate is timed twice per round: its two series are an A/A pair, and the distance of their medians is
the spread below which a difference says nothing.
  (a) stft_distance_many against torch.stft -> re^2 + im^2 -> clamp -> sqrt -> norms, log, mean on the GPU at the three default
      resolutions, and si_sdr_many + snr_many (two calls) against the direct torch form (alpha, then the residuals), with a Python
      loop over the clips where the lengths differ: 1 x 3 s, 64 x 3 s pairs, 200 pairs of 0.5 - 10 s.  The results are compared.
      Where the lengths are equal the compositions hold their (B, T) batches before the timed region.  Peak extra memory of each.
  (b) device time per case, events around the step, through the C ABI on buffers allocated beforehand, queued behind a spinning
      kernel so that the host's launch gaps stay outside, each twice (its own A/A pair): wt_stftd_distance and wt_wavedist.  With
      more than 64 pairs both brackets also hold the upload of the descriptors.
  (c) round_trip_report against round_trip_mel_distance, round_trip_stoi and three codec passes of one's own for the new measures
      (what a caller had to write before), on 64 x 3 s with the synthetic weights.
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
RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


def timed(fn, inner):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def pair(name, what, new, old, rounds, inner, log):
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
    log(f"  {name}: {what[0]} {new_ms:.4f} ms, {what[1]} {old_ms:.4f} ms, old / new {old_ms / new_ms:.3f}, A/A spread {aa:.4f} ms")
    return {"new_ms": round(new_ms, 4), "old_ms": round(old_ms, 4), "aa_spread_ms": round(aa, 4), "old_over_new": round(old_ms / new_ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-round-trip", action="store_true")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from wavtokenizer_amd import metrics
    from wavtokenizer_amd._capi import WtStftdClip, WtWavedistClip, check, lib
    res = {"rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    windows = [torch.hann_window(w, device="cuda") for _n, _h, w in RES]

    def mag(x, r):                                                      # (B, T) -> (B, bins, F)
        n_fft, hop, win = RES[r]
        Z = torch.stft(x, n_fft, hop, win, window=windows[r], center=True, pad_mode="reflect", return_complex=True)
        return torch.sqrt(torch.clamp(Z.real ** 2 + Z.imag ** 2, min=1e-7))

    def stft_rows(x, y):                                                # (B, T) pairs -> (B,)
        total = 0
        for r in range(len(RES)):
            X, Y = mag(x, r), mag(y, r)
            sc = torch.linalg.norm(Y - X, dim=(1, 2)) / torch.linalg.norm(Y, dim=(1, 2))
            total = total + sc + (torch.log(Y) - torch.log(X)).abs().mean(dim=(1, 2))
        return total / len(RES)

    def stft_composition(y_hats, ys):
        if isinstance(ys, torch.Tensor):
            return stft_rows(y_hats, ys)
        return torch.cat([stft_rows(p[None], q[None]) for p, q in zip(y_hats, ys)])

    eps = 2.0 ** -23

    def wave_rows(p, t):                                                # (B, T) pairs -> (B, 2)
        alpha = ((p * t).sum(-1, keepdim=True) + eps) / ((t * t).sum(-1, keepdim=True) + eps)
        at = alpha * t
        si = 10 * torch.log10(((at * at).sum(-1) + eps) / (((at - p) ** 2).sum(-1) + eps))
        sn = 10 * torch.log10(((t * t).sum(-1) + eps) / (((t - p) ** 2).sum(-1) + eps))
        return torch.stack([si, sn], dim=1)

    def wave_composition(ps, ts):
        if isinstance(ts, torch.Tensor):
            return wave_rows(ps, ts)
        return torch.cat([wave_rows(p[None], q[None]) for p, q in zip(ps, ts)])

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
    cases = (("1x3s", [3 * SR], 30), ("64x3s", [3 * SR] * 64, 5), ("200x0.5-10s", [int(v) for v in rng.integers(SR // 2, 10 * SR, 200)], 2))
    log(f"(a) stft_distance_many and si_sdr_many + snr_many against the torch compositions, (b) device time; {res['device']}")
    res["stft"], res["wave"], res["device_us"] = {}, {}, {}
    for name, lengths, inner in cases:
        ys = [torch.from_numpy((0.1 * rng.standard_normal(T)).astype(np.float32)).cuda() for T in lengths]
        y_hats = [y + 0.01 * torch.randn_like(y) for y in ys]
        batched = len(set(lengths)) == 1
        cy_hats, cys = (torch.stack(y_hats), torch.stack(ys)) if batched else (y_hats, ys)
        with torch.inference_mode():
            new, old = (lambda: metrics.stft_distance_many(y_hats, ys)), (lambda: stft_composition(cy_hats, cys))
            diff = float((new() - old()).abs().max())
            mem_new, mem_old = peak(new), peak(old)
            res["stft"][name] = pair("stft " + name, ("stft_distance_many", "torch composition"), new, old, a.rounds, inner, log)
            res["stft"][name].update(max_abs_diff=diff, peak_bytes_new=mem_new, peak_bytes_old=mem_old)
            log(f"  stft {name}: largest difference of a pair's distance {diff:.2e}; peak extra memory {mem_new / 2**20:.2f} MiB against {mem_old / 2**20:.2f} MiB")
            new = lambda: (metrics.si_sdr_many(y_hats, ys), metrics.snr_many(y_hats, ys))
            old = lambda: wave_composition(cy_hats, cys)
            got, want = new(), old()
            diff = float(max((got[0] - want[:, 0]).abs().max(), (got[1] - want[:, 1]).abs().max()))
            mem_new, mem_old = peak(new), peak(old)
            res["wave"][name] = pair("wave " + name, ("si_sdr_many + snr_many", "torch composition"), new, old, a.rounds, inner * 2, log)
            res["wave"][name].update(max_abs_diff_db=diff, peak_bytes_new=mem_new, peak_bytes_old=mem_old)
            log(f"  wave {name}: largest difference {diff:.2e} dB; peak extra memory {mem_new / 2**20:.2f} MiB against {mem_old / 2**20:.2f} MiB")
            # (b) the C ABI on buffers allocated here
            n = len(ys)
            frames = sum(1 + T // hop for T in lengths for _n, hop, _w in RES)
            h = metrics.stftd_handle(RES, 0)
            dist = torch.empty((n, 7), dtype=torch.float32, device="cuda")
            both = torch.empty((n, 2), dtype=torch.float32, device="cuda")
            ws = torch.empty(int(lib.wt_stftd_workspace_bytes(h, n, frames)) // 8 + 1, dtype=torch.int64, device="cuda")
            ws2 = torch.empty(int(lib.wt_wavedist_workspace_bytes(n, sum(lengths))) // 8 + 1, dtype=torch.int64, device="cuda")
            d_st, d_wd = (WtStftdClip * n)(), (WtWavedistClip * n)()
            for i in range(n):
                d_st[i].estimate, d_st[i].target, d_st[i].length, d_st[i].out = y_hats[i].data_ptr(), ys[i].data_ptr(), lengths[i], dist.data_ptr() + 28 * i
                d_wd[i].estimate, d_wd[i].target, d_wd[i].length, d_wd[i].out = y_hats[i].data_ptr(), ys[i].data_ptr(), lengths[i], both.data_ptr() + 8 * i
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            st_call = lambda: check(lib.wt_stftd_distance(h, d_st, n, ctypes.c_void_p(ws.data_ptr()), stream), "wt_stftd_distance")
            wd_call = lambda: check(lib.wt_wavedist(d_wd, n, 0, ctypes.c_void_p(ws2.data_ptr()), stream), "wt_wavedist")
            dev = {"wt_stftd_distance": [device_us(st_call) for _ in range(2)], "wt_wavedist": [device_us(wd_call) for _ in range(2)]}
            assert torch.equal(dist[:, 0], metrics.stft_distance_many(y_hats, ys)) and torch.equal(both[:, 0], metrics.si_sdr_many(y_hats, ys))
            res["device_us"][name] = dict(dev, frames=frames, samples=sum(lengths))
            log(f"  {name}: device time, events around the step: wt_stftd_distance ({frames} frames of both signals) {dev['wt_stftd_distance'][0]:.2f} / "
                f"{dev['wt_stftd_distance'][1]:.2f} us, {dev['wt_stftd_distance'][1] * 1e3 / frames:.2f} ns per frame pair; wt_wavedist ({sum(lengths)} samples) "
                f"{dev['wt_wavedist'][0]:.2f} / {dev['wt_wavedist'][1]:.2f} us")
    if not a.skip_round_trip:
        from tests.util import synth_state_dict
        from wavtokenizer_amd import ARCH_HOP600, WavTokenizer, synth
        m = WavTokenizer.from_arch(ARCH_HOP600)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict("hop600").items()}, strict=False)
        m = m.eval().to("cuda")
        wavs = [torch.from_numpy(c).cuda() for c in synth.make_clips(64, 3 * SR, seed=9)]
        bw = torch.tensor([0])

        def crops():
            outs = m.decode_codes_many(m.encode_codes_many(wavs, bandwidth_id=bw), bandwidth_id=bw)
            return [o[0, :w.shape[0]] for o, w in zip(outs, wavs)]

        def separate():
            return (m.round_trip_mel_distance(wavs, bandwidth_id=bw), m.round_trip_stoi(wavs, bandwidth_id=bw),
                    metrics.stft_distance_many(crops(), wavs), metrics.si_sdr_many(crops(), wavs), metrics.snr_many(crops(), wavs))

        with torch.inference_mode():
            rep, sep = m.round_trip_report(wavs, bandwidth_id=bw), separate()
            same = all(torch.equal(rep[k], v) for k, v in zip(("mel_distance", "stoi", "stft_distance", "si_sdr", "snr"), sep))
            log(f"(c) round_trip_report against the five separate round trips, 64 x 3 s, synthetic weights; equal bits: {same}")
            res["round_trip"] = pair("report 64x3s", ("round_trip_report", "five separate round trips"),
                                     lambda: m.round_trip_report(wavs, bandwidth_id=bw), separate, a.rounds, 1, log)
            res["round_trip"]["equal_bits"] = bool(same)
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
