#!/usr/bin/env python3
"""Per-clip level control: what normalising on ingest and rescaling on emit cost against the compositions they replace, whether
the default path moved, and the device time of the new launches.
python3 tools/level_bench.py [--rounds 7] [--prev tools/lib/libwavtok_hip_prev.so] [--out profiles/level_bench.txt]

  (a) encode_codes_many(normalize="peak") against the composition per file: audio.convert_audio, the torch expression
      x / (x.abs().max() + 1e-8), then encode_infer_many
  (b) decode_pcm_many(rescale=True) to int16 against decode_pcm_many(dtype=fp32) followed by audio.to_pcm16(rescale=True) per clip
  (c) the default path, encode_codes_many and decode_pcm_many with no new argument, this build against the parent commit's library
      (tools/build_prev.sh), in child processes alternating prev, new, prev, new
  (d) the device time of wt_level, wt_normalize_rows and wt_emit_rescaled at 64 x 3 s, HIP events around the call
(a) and (b) at 1 x 3 s, 64 x 3 s and 200 clips of 0.5 - 10 s at five rates; (c) at 64 x 3 s and at the 200 clips.

One process per library, every plan and graph warm before anything is timed.  Per case the two candidates alternate round by round
and each is timed TWICE per round (new, old, new, old): the two series of one candidate are an A/A pair, and the distance of their
medians is the spread below which a difference says nothing.  A sample is `inner` calls and one stream synchronise, with
set_strict_status(False) and set_check_codes("off").  Both candidates are checked to return the same bits."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 24000
RATES = [16000, 22050, 24000, 44100, 48000]


def timed(fn, inner):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def model():
    import torch
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth
    arch = NAMED_ARCHS["hop600"]
    m = WavTokenizer.from_arch(arch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(arch, seed=0).items()}, strict=False)
    m = m.eval().cuda()
    m.set_strict_status(False)
    m.set_check_codes("off")
    return m


def workloads(files, seed=0):
    """name -> (clips on the GPU, their rates, codes per clip, inner calls per sample)."""
    import numpy as np
    import torch
    from wavtokenizer_amd import synth
    rng = np.random.default_rng(seed)
    out = {}
    for name, B, inner in (("1x3s", 1, 30), ("64x3s", 64, 5)):
        wav = torch.from_numpy(synth.make_clips(B, 3 * SR, seed=10 + B) * np.float32(0.1)).cuda()
        out[name] = ([w for w in wav], [SR] * B, [torch.from_numpy(rng.integers(0, 4096, size=(1, 3 * SR // 600))).cuda() for _ in range(B)], inner)
    clips, rates, codes = [], [], []
    for i in range(files):
        sr = int(rng.choice(RATES))
        sec = float(rng.uniform(0.5, 10.0))
        clips.append(torch.from_numpy(synth.make_clips(1, int(sec * sr), seed=100 + i, sample_rate=sr)[0] * np.float32(0.1)).cuda())
        rates.append(sr)
        codes.append(torch.from_numpy(rng.integers(0, 4096, size=(1, max(1, int(sec * SR / 600))))).cuda())
    out[f"{files}_mixed"] = (clips, rates, codes, 1)
    return out


def child(rounds, files):
    """(c), one library: medians of the default encode_codes_many / decode_pcm_many, as one JSON line."""
    import numpy as np
    import torch
    m = model()
    bw = torch.tensor([0])
    out = {}
    for name, (clips, rates, codes, inner) in workloads(files).items():
        if name == "1x3s":
            continue
        enc = lambda: m.encode_codes_many(clips, sample_rates=rates, packed=True)[0]
        dec = lambda: m.decode_pcm_many(codes, sample_rates=rates, packed=True, bandwidth_id=bw)[0]
        for tag, fn in (("encode", enc), ("decode", dec)):
            for _ in range(3):
                fn()
            out[f"{tag}_{name}"] = float(np.median([timed(fn, inner) for _ in range(rounds)]))
            out[f"{tag}_{name}_sum"] = int(fn().long().sum())
    m.check_status()
    print("CHILD " + json.dumps(out), flush=True)


def run_child(lib, rounds, files):
    env = dict(os.environ)
    if lib:
        env["WAVTOK_HIP_LIB"] = lib
    else:
        env.pop("WAVTOK_HIP_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(rounds), "--files", str(files)], env=env,
                       capture_output=True, text=True, timeout=500)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")]
    if p.returncode or not line:
        raise RuntimeError(f"child with {lib or 'this build'} failed ({p.returncode}): {p.stderr[-600:]}")
    return json.loads(line[-1][6:])


def pair(name, new, old, rounds, inner, same, log):
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
    log(f"  {name}: new {new_ms:.4f} ms, composition {old_ms:.4f} ms, old / new {old_ms / new_ms:.3f}, A/A spread {aa:.4f} ms"
        f"{'' if same else '; OUTPUTS DIFFER'}")
    return {"new_ms": round(new_ms, 4), "old_ms": round(old_ms, 4), "aa_spread_ms": round(aa, 4), "old_over_new": round(old_ms / new_ms, 3),
            "identical_outputs": bool(same)}


def event_ms(call, reps):
    """Mean device time of call() between two HIP events on the current stream, over reps calls."""
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        call()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--prev", default=os.path.join(ROOT, "tools", "lib", "libwavtok_hip_prev.so"))
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.rounds, a.files)
        return 0
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    res = {"rounds": a.rounds}
    # ---- (c): before this process opens the GPU, so that one process at a time times on it
    log("(c) the default path (no new argument): this build against the parent commit's library, child processes alternating prev, new, prev, new")
    if os.path.exists(a.prev):
        runs = [(tag, run_child(lib, a.rounds, a.files)) for tag, lib in (("prev", a.prev), ("new", ""), ("prev", a.prev), ("new", ""))]
        res["c"] = {}
        for key in [k for k in runs[0][1] if not k.endswith("_sum")]:
            p, n = [r[key] for t, r in runs if t == "prev"], [r[key] for t, r in runs if t == "new"]
            same = len({r[key + "_sum"] for _t, r in runs}) == 1
            aa = max(abs(p[0] - p[1]), abs(n[0] - n[1]))
            diff = sum(n) / 2 - sum(p) / 2
            log(f"  {key:18s}: prev {p[0]:.4f} {p[1]:.4f} ms, new {n[0]:.4f} {n[1]:.4f} ms, new - prev {diff:+.4f} ms, A/A spread {aa:.4f} ms -> "
                f"{'inside the spread' if abs(diff) <= aa else 'OUTSIDE the spread'}{'' if same else '; OUTPUTS DIFFER'}")
            res["c"][key] = {"prev_ms": [round(v, 4) for v in p], "new_ms": [round(v, 4) for v in n], "aa_spread_ms": round(aa, 4),
                             "new_minus_prev_ms": round(diff, 4), "same_outputs": same}
    else:
        log(f"  not measured: {a.prev} is missing (tools/build_prev.sh builds it)")

    import torch
    from wavtokenizer_amd import _capi, audio
    m = model()
    bw = torch.tensor([0])
    res["device"] = torch.cuda.get_device_name(0)
    loads = workloads(a.files)

    log(f"(a) encode_codes_many(normalize='peak') against convert_audio + the torch expression per file + encode_infer_many, {res['device']}")
    res["a"] = {}
    for name, (clips, rates, _codes, inner) in loads.items():
        def old():
            ws = []
            for c, sr in zip(clips, rates):
                w = audio.convert_audio(c[None, None], sr, SR, 1)[0, 0] if sr != SR else c
                ws.append(w / (w.abs().max() + 1e-8))
            return torch.cat([c.view(-1) for _f, c in m.encode_infer_many(ws, bandwidth_id=bw)])
        new = lambda: m.encode_codes_many(clips, sample_rates=rates, packed=True, normalize="peak")[0]
        res["a"][name] = pair(name, new, old, a.rounds, inner, torch.equal(new(), old()), log)

    log("(b) decode_pcm_many(rescale=True) to int16 against decode_pcm_many(dtype=fp32) + to_pcm16(rescale=True) per clip")
    res["b"] = {}
    for name, (_clips, rates, codes, inner) in loads.items():
        new = lambda: m.decode_pcm_many(codes, sample_rates=rates, packed=True, bandwidth_id=bw, rescale=True)[0]
        old = lambda: torch.cat([audio.to_pcm16(r, rescale=True).view(-1)
                                 for r in m.decode_pcm_many(codes, sample_rates=rates, dtype=torch.float32, bandwidth_id=bw)])
        res["b"][name] = pair(name, new, old, a.rounds, inner, torch.equal(new(), old()), log)

    log("(d) device time at 64 x 3 s, HIP events around 20 calls (each figure twice: its own A/A pair)")
    B, T = 64, 3 * SR
    rows = torch.randn(B, T, device="cuda") * 0.1
    out = torch.empty(B, 2, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    lv = (_capi.WtLevelClip * B)()
    for j, d in enumerate(lv):
        d.x, d.n, d.out = rows[j].data_ptr(), T, out.data_ptr() + 8 * j
    ws_l = torch.empty(int(_capi.lib.wt_level_workspace_bytes(B, B * T)), dtype=torch.uint8, device="cuda")
    ws_n = torch.empty(int(_capi.lib.wt_normalize_rows_workspace_bytes(B, T)), dtype=torch.uint8, device="cuda")
    scales = torch.empty(B, device="cuda")
    n = (ctypes.c_int64 * B)(*[T] * B)
    pcm = torch.empty(B, T, dtype=torch.int16, device="cuda")
    em = (_capi.WtEmitClip * B)()
    for j, d in enumerate(em):
        d.src, d.n_in, d.resampler, d.n_out, d.dst = rows[j].data_ptr(), T, audio.resampler(SR, SR, 0), T, pcm[j].data_ptr()
        d.dtype, d.channels, d.ch_stride, d.sample_stride, d.limit = _capi.WT_EMIT_I16, 1, 0, 1, 0.05
    ws_e = torch.empty(int(_capi.lib.wt_emit_rescaled_workspace_bytes(B)), dtype=torch.uint8, device="cuda")
    calls = {"wt_level": lambda: _capi.check(_capi.lib.wt_level(lv, B, ptr(ws_l), stream)),
             "wt_normalize_rows": lambda: _capi.check(_capi.lib.wt_normalize_rows(ptr(rows), B, T, n, 0, 1.0, ptr(scales), ptr(ws_n), stream)),
             "wt_emit_rescaled": lambda: _capi.check(_capi.lib.wt_emit_rescaled(em, B, ptr(ws_e), stream)),
             "wt_emit": lambda: _capi.check(_capi.lib.wt_emit(em, B, ptr(ws_e), stream))}
    res["d"] = {}
    for rep in ("first", "again"):
        for name, call in calls.items():
            us = event_ms(call, 20) * 1e3
            res["d"].setdefault(name, {})[rep] = round(us, 2)
            log(f"  {name:18s} {rep:5s}: {us:8.2f} us per call ({B * T * 4 / 1e6:.1f} MB of fp32 samples)")
    m.check_status()
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ok = all(v.get("identical_outputs", True) for k in ("a", "b") for v in res[k].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
