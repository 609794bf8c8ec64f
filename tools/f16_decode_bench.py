#!/usr/bin/env python3
"""The one-product GEMM mode of the decoder, set_gemm_precision("f16"), against the default "f16x3", on decode_codes.
python3 tools/f16_decode_bench.py [--arch hop600] [--rounds 7] [--seed 0] [--out profiles/f16_decode_bench.txt]

One process, one model; the mode is toggled between calls (plans are cached per flag set), every plan and graph warm before
anything is timed.  Three cases:
  (a) B = 1, L = 120 frames, graph replay
  (b) B = 64, L = 120
  (c) B = 32, L = 1200
Per case the two candidates alternate round by round, and each is timed TWICE per round (new, old, new, old; new = "f16"): the
two series of one candidate are an A/A pair, and the larger distance of their medians is the spread below which a difference
between the candidates says nothing.  A sample is `inner` calls and one stream synchronise.  The model runs with
set_check_codes("off") and set_strict_status(False): a sample holds launches and no per-call synchronise.  Then, at shape (b),
the time of the steps cnx.pwconv1, head.out, head.istft and attn.s under both modes, taken on the device by the launches
themselves (wt_plan_set_timing("@name")), and the relative L2 distance of the two modes' waveforms.  Prints one line per
series, one verdict per case and one JSON line at the end."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, _capi, synth  # noqa: E402


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def compare(name, new, old, rounds, inner, log):
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
    aa_new, aa_old = abs(med["new"] - med["new_again"]), abs(med["old"] - med["old_again"])
    faster = old_ms - new_ms > max(aa_new, aa_old)
    log(f"  {name}: f16 {new_ms:.4f} ms, f16x3 {old_ms:.4f} ms, f16x3 / f16 {old_ms / new_ms:.3f}, difference {old_ms - new_ms:+.4f} ms, "
        f"A/A spreads {aa_new:.4f} / {aa_old:.4f} ms -> {'f16 FASTER by more than both spreads' if faster else 'no gain beyond the spread'}")
    return {"f16_ms": round(new_ms, 4), "f16x3_ms": round(old_ms, 4), "aa_spread_f16_ms": round(aa_new, 4), "aa_spread_f16x3_ms": round(aa_old, 4),
            "f16x3_over_f16": round(old_ms / new_ms, 3), "faster_beyond_both_spreads": bool(faster),
            "medians_ms": {k: round(v, 4) for k, v in med.items()}}


def step_times(m, run, B, L, f16, steps, calls=10):
    """us per launch of each named gemm16s step of the decode-from-codes plan (B, L) of one mode, timed on the device."""
    flag = _capi.WT_PLAN_FLAG_F16_GEMM
    (plan, _ws), = [v for k, v in m._engine.plans.items()
                    if k[0] == _capi.WT_PLAN_DECODE_CODES and k[1] == B and k[2] == L and bool(k[3] & flag) == f16]
    out = {}
    for name in steps:
        _capi.check(_capi.lib.wt_plan_set_timing(plan, b"@" + name.encode()), "wt_plan_set_timing")
        for _ in range(calls):
            run()
        tot, n = ctypes.c_double(), ctypes.c_int64()
        _capi.check(_capi.lib.wt_plan_read_timing(plan, ctypes.byref(tot), ctypes.byref(n), 1), "wt_plan_read_timing")
        _capi.lib.wt_plan_set_timing(plan, b"")
        out[name] = {"us_per_launch": round(1e3 * tot.value / max(n.value, 1), 2), "launches_per_call": n.value // calls}
    return out


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
    log(f"decode_codes under set_gemm_precision(\"f16\") against \"f16x3\": {a.arch}, {res['device']}, {a.rounds} rounds")

    def in_mode(mode, c):
        def run():
            m.set_gemm_precision(mode)
            return m.decode_codes(c, bandwidth_id=bw)
        return run

    keep = {}
    for case, B, L, inner in (("a", 1, 120, 50), ("b", 64, 120, 10), ("c", 32, 1200, 3)):
        c = torch.from_numpy(rng.integers(0, arch.vq_bins, size=(1, B, L))).cuda()
        new, old = in_mode("f16", c), in_mode("f16x3", c)
        log(f"({case}) B = {B}, L = {L}{', graph replay' if B <= m._graph_max_clips else ''}")
        res[case] = compare(case, new, old, a.rounds, inner, log)
        wn, wo = new().double(), old().double()
        res[case]["rel_l2_f16_from_f16x3"] = float(((wn - wo) ** 2).sum().sqrt() / (wo ** 2).sum().sqrt())
        log(f"  {case}: waveform of f16 at rel-L2 {res[case]['rel_l2_f16_from_f16x3']:.3e} from f16x3")
        keep[case] = (new, old, B, L)

    new, old, B, L = keep["b"]
    steps = ("cnx.pwconv1", "head.out", "head.istft", "attn.s")
    res["steps_b"] = {"f16": step_times(m, new, B, L, True, steps), "f16x3": step_times(m, old, B, L, False, steps)}
    log(f"per-launch time of the steps at B = {B}, L = {L} (device clock, first entry to last exit of the launch):")
    for s in steps:
        n, o = res["steps_b"]["f16"][s], res["steps_b"]["f16x3"][s]
        log(f"  {s:12s}: f16 {n['us_per_launch']:8.2f} us   f16x3 {o['us_per_launch']:8.2f} us   ({o['launches_per_call']} launches per call)")
    m.set_gemm_precision("f16x3")
    m.check_status()
    log(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
