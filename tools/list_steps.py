"""Plan signatures: one JSON line per plan of a fixed list of plan variants (both architectures, B = 2) with its step
names in order, wt_plan_num_launches, wt_plan_workspace_bytes, its buffers as (name, numel, format) and the SHA-256 of
every output for seeded synthetic weights and inputs.  A plan refactor keeps every line as it was: run this once per
library (WAVTOK_HIP_LIB names the one to load) and diff the two outputs.

    python tools/list_steps.py > new.jsonl
    WAVTOK_HIP_LIB=tools/lib/libwavtok_hip_prev.so python tools/list_steps.py > prev.jsonl

"repeatable" says whether a second call on the same plan gave the same hashes.  Graph replay is off: it changes how a
plan's launches are issued, not which."""
import ctypes, hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from wavtokenizer_amd import WavTokenizer, NAMED_ARCHS, synth, _capi
from wavtokenizer_amd._capi import lib

B, T, T_SHORT = 2, 24000, 900          # T_SHORT: below the fused stage-1 down conv's 1024-sample minimum
BW = torch.tensor([0])
F = _capi


def sha(x) -> str:
    a = x.detach().cpu().contiguous().numpy() if isinstance(x, torch.Tensor) else x
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def plan_signature(plan) -> dict:
    steps = []
    for i in range(lib.wt_plan_num_steps(plan)):
        p = ctypes.c_char_p()
        assert lib.wt_plan_step_name(plan, i, ctypes.byref(p)) == 0
        steps.append(p.value.decode())
    bufs, i, p = [], 0, ctypes.c_char_p()
    while lib.wt_plan_buffer_name(plan, i, ctypes.byref(p)) == 0:
        off, n, fmt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
        assert lib.wt_plan_buffer_info(plan, p.value, ctypes.byref(off), ctypes.byref(n), ctypes.byref(fmt)) == 0
        bufs.append([p.value.decode(), n.value, fmt.value])
        i += 1
    return {"steps": steps, "launches": lib.wt_plan_num_launches(plan),
            "workspace_bytes": lib.wt_plan_workspace_bytes(plan), "buffers": bufs}


def range_entries(plan) -> list:
    out, i = [], 0
    step, buf, amax = ctypes.c_char_p(), ctypes.c_char_p(), ctypes.c_float()
    while lib.wt_plan_range_report(plan, i, ctypes.byref(step), ctypes.byref(buf), ctypes.byref(amax)) == 0:
        out.append([step.value.decode(), buf.value.decode(), float(amax.value)])
        i += 1
    return out


def main():
    dev = torch.device("cuda")
    for arch_name, arch in NAMED_ARCHS.items():
        sd = synth.make_state_dict(arch, seed=0, with_seanet_decoder=True)
        m = WavTokenizer.from_arch(arch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        m = m.eval().to(dev)
        m.set_graph_max_clips(0)
        L = arch.frames(T)
        g = torch.Generator().manual_seed(3)
        wav = torch.from_numpy(synth.make_clips(B, T, seed=1)).to(dev)
        codebook = torch.from_numpy(sd["feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed"])
        feats = codebook[torch.randint(0, arch.vq_bins, (B, L), generator=g)].permute(0, 2, 1).contiguous().to(dev)
        bb = torch.randn(B, L, arch.dim, generator=g).to(dev)
        lstm_in = (0.5 * torch.randn(B, L, 512, generator=g)).to(dev)
        runs = {     # plan kind -> (length, call returning the named outputs)
            "encode": (T, lambda: dict(zip(("feats", "codes", "emb"), m._run_encode(wav)))),
            "encode_short": (T_SHORT, lambda: dict(zip(("feats", "codes", "emb"), m._run_encode(wav[:, :T_SHORT])))),
            "decode": (L, lambda: dict(zip(("wav", "backbone"), m._run_decode(feats, BW, want_backbone=True)))),
            "seanet_decoder": (L, lambda: {"wav": m._run_seanet_decoder(feats)}),
            "head": (L, lambda: {"wav": m._run_head(bb)}),
            "unit_lstm": (L, lambda: {"y": m._run_unit_lstm(lstm_in)}),
        }
        kinds = {"encode": F.WT_PLAN_ENCODE, "encode_short": F.WT_PLAN_ENCODE, "decode": F.WT_PLAN_DECODE,
                 "seanet_decoder": F.WT_PLAN_SEANET_DECODER, "head": F.WT_PLAN_HEAD, "unit_lstm": F.WT_PLAN_UNIT_LSTM}
        dec_sites = [F.WT_SITE_BB_EMBED, F.WT_SITE_RES0, F.WT_SITE_RES1, F.WT_SITE_ATTN, F.WT_SITE_RES2, F.WT_SITE_RES3,
                     *(F.WT_SITE_CNX0 + i for i in range(arch.num_layers)), F.WT_SITE_HEAD]
        KEEP, FP32, STEP, UNF, RR = (F.WT_PLAN_FLAG_KEEP_STAGES, F.WT_PLAN_FLAG_FP32_GEMM, F.WT_PLAN_FLAG_STEP_LSTM,
                                     F.WT_PLAN_FLAG_UNFUSED, F.WT_PLAN_FLAG_RANGE_REPORT)
        variants = [     # (run, variant name, plan flags, fp32 sites)
            ("encode", "default", 0, []), ("encode", "FP32_GEMM", FP32, []), ("encode", "KEEP_STAGES", KEEP, []),
            ("encode", "KEEP_STAGES|UNFUSED", KEEP | UNF, []), ("encode", "STEP_LSTM", STEP, []),
            ("encode", "RANGE_REPORT", RR, []), ("encode_short", "default", 0, []),
            ("decode", "default", 0, []), ("decode", "FP32_GEMM", FP32, []), ("decode", "KEEP_STAGES|UNFUSED", KEEP | UNF, []),
            ("decode", "sites=BB_EMBED", 0, [F.WT_SITE_BB_EMBED]), ("decode", "sites=RES1", 0, [F.WT_SITE_RES1]),
            ("decode", "sites=ATTN", 0, [F.WT_SITE_ATTN]), ("decode", "sites=CNX0+3", 0, [F.WT_SITE_CNX0 + 3]),
            ("decode", "sites=HEAD", 0, [F.WT_SITE_HEAD]), ("decode", "sites=all", 0, dec_sites),
            ("seanet_decoder", "default", 0, []), ("seanet_decoder", "FP32_GEMM", FP32, []),
            ("seanet_decoder", "UNFUSED", UNF, []),
            ("head", "default", 0, []), ("head", "FP32_GEMM", FP32, []),
            ("unit_lstm", "default", 0, []), ("unit_lstm", "STEP_LSTM", STEP, []),
        ]
        for run, name, flags, sites in variants:
            length, call = runs[run]
            kind = kinds[run]
            m._plan_flags = flags
            m._fp32_sites = sum(1 << s for s in sites)
            hashes = [{k: sha(v) for k, v in call().items()} for _ in range(2)]
            torch.cuda.synchronize()
            plan = m._engine.plans[m._engine._key(kind, B, length, flags, dev, m._sites(kind))][0]
            sig = {"arch": arch_name, "plan": run, "variant": name, "B": B, "len": length, **plan_signature(plan),
                   "outputs": hashes[0], "repeatable": hashes[0] == hashes[1]}
            if flags & RR:
                sig["outputs"]["range_report"] = sha(np.frombuffer(json.dumps(range_entries(plan)).encode(), np.uint8))
            print(json.dumps(sig), flush=True)
            m._engine.drop(lambda k: True)
        m._plan_flags, m._fp32_sites = 0, 0
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
