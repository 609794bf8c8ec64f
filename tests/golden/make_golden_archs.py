#!/usr/bin/env python3
"""Fixtures for architectures OTHER than the two the reference ships YAMLs for, from the REAL reference.

wt_model_create takes a family of architectures (dim 256 .. 1024, any intermediate_dim % 32, depths to 32, any codebook size % 4,
any four ratios to 16, n_fft an even multiple of hop_length); every other end-to-end fixture is hop600 or hop320.  Three variants
(VARIANTS below) reach the shape-dependent decisions of the plans that those two never take.  For each one the hop-600 YAML's
three init_args blocks are replaced by ArchConfig.to_yaml_node() (written to a temporary file, nothing of it is kept), the
reference is built from it with the synthetic weights, and the script asserts before it writes anything that
  - arch_from_yaml_dict() of that YAML gives the variant back,
  - oracle/cpu_ref.py is bit-identical to the reference for features, codes, waveform and every tap (inference_mode),
  - every frame's FLOAT64 top-2 margin exceeds tests/util.py NEAR_TIE_MARGIN (else the next clip seed is taken: no frame is
    ever excused) and the fp32 codes are the float64 codes.
Weights (synth.make_state_dict(arch, weight_seed)) and clips (synth.make_clips(B, T, seed)) are regenerated at test time.

    python tests/golden/make_golden_archs.py        # where the reference checkout is (make_golden.py YAMLS), not at test time
"""
import json
import os
import sys
import tempfile
import warnings

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

from wavtokenizer_amd import synth  # noqa: E402
from wavtokenizer_amd.config import ArchConfig, arch_from_yaml_dict  # noqa: E402
from oracle.cpu_ref import OracleWavTokenizer  # noqa: E402
from tests.util import NEAR_TIE_MARGIN, manifest  # noqa: E402
from _ref_import import build_reference  # noqa: E402
from make_golden import YAMLS, check_identical  # noqa: E402

VARIANTS = {
    # first encoder ratio 3 (no fused stage-1 down kernel at any T), K/32 = 3 on pwconv2, N = 96, a codebook narrower than one
    # argmax tile, R = 2, rownorm<1>, one AdaLN row
    "narrow": ArchConfig(ratios=(5, 4, 4, 3), vq_bins=8, dim=256, intermediate_dim=96, num_layers=1, adanorm_num_embeddings=1,
                         n_fft=480, hop_length=240),
    # a down conv with k = 32, the most taps the GEMM kernels gather and the largest tap-paired conv; first encoder ratio 5 (no
    # fused stage-1 down kernel; with ratios ending in 2 no clip seed of 200 kept every float64 margin above the bar), K/32 = 47 (odd), vq_bins no multiple of 192, R = 6, Kq = 736, rownorm<2>.
    # (Planned with ratios (20, 3, 2, 4): its down conv has k = 40 taps, which neither GEMM engine gathers; the model loaded and
    # its encode failed at that launch.  Ratios above 16 are now refused at load: tests/test_arch_variants_host.py REFUSALS.)
    "mid16": ArchConfig(ratios=(16, 3, 2, 5), vq_bins=1024, dim=512, intermediate_dim=1504, num_layers=3, adanorm_num_embeddings=4,
                        n_fft=2880, hop_length=480),
    # the largest ratio in the LAST place (the first encoder stage): its down conv (32 -> 64 channels, k = 32) runs as a GEMM with
    # N = 64, whose 256-row tile has no room for the offset tables of more than 19 taps; the 128-row tile takes it.  narrow's
    # other sizes (one architecture per question)
    "last16": ArchConfig(ratios=(5, 3, 4, 16), vq_bins=8, dim=256, intermediate_dim=96, num_layers=1, adanorm_num_embeddings=1,
                         n_fft=1920, hop_length=960),
    # rownorm<4>, GroupNorm group width 32, N = 2080 (no multiple of 128 or 192), the reference's default codebook size
    # (85.3 argmax tiles), three AdaLN rows
    "wide": ArchConfig(ratios=(8, 5, 4, 2), vq_bins=16384, dim=1024, intermediate_dim=2080, num_layers=2, adanorm_num_embeddings=3,
                       n_fft=1280, hop_length=320),
}
CLIP_SEED0 = 77
HEAD = 4                 # time steps kept from the start of clip 0 of every tap
MAX_FILE = 1 << 20
MAX_TOTAL = 4 << 20


def cases_of(arch):
    """(name, B, T, bandwidth_id): `small` = 6 frames with a ragged last hop; `rows` = L = 130 (across 128) and 1040 GEMM rows."""
    hop = arch.hop
    return (("small", 2, 5 * hop + 17, arch.adanorm_num_embeddings - 1), ("rows", 8, 129 * hop + 1, 0))


def ref_taps(ref, arch):
    """Forward hooks on the reference's modules under the oracle's tap names (make_golden.ref_taps for any depth)."""
    taps, hooks = {}, []

    def add(mod, name, post=None):
        def fn(_m, _i, o):
            taps[name] = post(o) if post else o
        hooks.append(mod.register_forward_hook(fn))

    enc = ref.feature_extractor.encodec.encoder.model
    for i in range(len(enc)):
        if type(enc[i]).__name__ in ("SConv1d", "SEANetResnetBlock", "SLSTM"):
            add(enc[i], f"enc.{i}")
    bb = ref.backbone
    add(bb.embed, "bb.embed")
    for i in range(6):
        add(bb.pos_net[i], f"bb.pos_net.{i}")
    add(bb.norm, "bb.norm", post=lambda o: o.transpose(1, 2))
    for i in sorted({0, arch.num_layers // 2 - 1, arch.num_layers - 1} - {-1}):
        add(bb.convnext[i], f"bb.convnext.{i}")
    add(bb.final_layer_norm, "bb.out")
    add(ref.head.out, "head.out", post=lambda o: o.transpose(1, 2))
    return taps, hooks


def run_case(ref, orc, o64, arch, B, T, bw_id, seed):
    """The reference and both oracles on one seeded batch; None when a float64 margin is a near tie."""
    wav = torch.from_numpy(synth.make_clips(B, T, seed))
    bw = torch.tensor([bw_id])
    with torch.inference_mode():
        t64 = {}
        _f64, c64 = o64.encode_infer(wav.double(), bw, t64)
        margin = t64["vq.margin"].numpy()
        if float(margin.min()) <= NEAR_TIE_MARGIN:
            return None
        rt, hooks = ref_taps(ref, arch)
        feats_r, codes_r = ref.encode_infer(wav, bandwidth_id=bw)
        wav_r = ref.decode(feats_r, bandwidth_id=bw)
        for h in hooks:
            h.remove()
        ot = {}
        feats_o, codes_o = orc.encode_infer(wav, bw, ot)
        wav_o = orc.decode(feats_o, bw, ot)
        feats2_r = ref.codes_to_features(codes_r)
    check_identical("features", feats_o, feats_r)
    check_identical("codes", codes_o, codes_r)
    check_identical("codes_to_features==features", feats2_r, feats_r)
    check_identical("waveform", wav_o, wav_r)
    assert set(rt) == {k for k in ot if k != "vq.margin"}, (sorted(rt), sorted(ot))
    for k, v in rt.items():
        check_identical(k, ot[k], v)
    if not torch.equal(codes_r, c64):
        return None                                 # (cannot happen above the margin bar short of a real fp32 problem)
    L = arch.frames(T)
    assert tuple(codes_r.shape) == (1, B, L) and tuple(wav_r.shape) == (B, L * arch.hop_length)
    out = {"codes": codes_r.numpy(), "margin": margin.astype(np.float64)}
    for k, v in rt.items():
        a = v.numpy()
        out[f"tap/{k}/shape"] = np.array(a.shape)
        out[f"tap/{k}/l2"] = np.float64(np.sqrt((a.astype(np.float64) ** 2).sum()))
        out[f"tap/{k}/head"] = (a[0, :HEAD] if k == "bb.out" else a[0, :, :HEAD]).copy()      # bb.out is (B, L, C)
    w = wav_r.numpy()
    out["wav_out_l2"] = np.sqrt((w.astype(np.float64) ** 2).sum(axis=1))
    out["wav_out"] = w if B <= 2 else w[:1]         # the large case: clip 0 in full, the norm of every clip
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    with open(YAMLS["hop600"]) as f:
        base_cfg = yaml.safe_load(f)
    weight_seed = manifest()["weight_seed"]
    total = 0
    for name, arch in VARIANTS.items():
        cfg = json.loads(json.dumps(base_cfg))
        node = arch.to_yaml_node()
        for k in ("feature_extractor", "backbone", "head"):
            cfg["model"]["init_args"][k] = node[k]
        assert arch_from_yaml_dict(cfg) == arch, f"{name}: arch_from_yaml_dict does not give the variant back"
        sd = synth.make_state_dict(arch, seed=weight_seed)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, f"{name}.yaml")
            with open(path, "w") as f:
                yaml.safe_dump(cfg, f)
            ref = build_reference(path, sd)
        orc = OracleWavTokenizer(arch, sd)
        o64 = OracleWavTokenizer(arch, {k: torch.from_numpy(v).double() for k, v in sd.items()})
        flat = {"arch": np.array(json.dumps(arch.to_dict())), "head_steps": np.int64(HEAD)}
        table = []
        for case, B, T, bw_id in cases_of(arch):
            seed = CLIP_SEED0
            while True:
                res = run_case(ref, orc, o64, arch, B, T, bw_id, seed)
                if res is not None:
                    break
                seed += 1
                if seed > CLIP_SEED0 + 200:
                    raise SystemExit(f"{name}/{case}: no clip seed whose every float64 margin exceeds {NEAR_TIE_MARGIN}")
            assert float(res["margin"].min()) > NEAR_TIE_MARGIN
            for k, v in res.items():
                flat[f"{case}/{k}"] = v
            table.append((case, B, T, seed, bw_id))
            print(f"{name}/{case}: B {B} T {T} frames {arch.frames(T)} bandwidth_id {bw_id} clip seed {seed} "
                  f"min float64 margin {float(res['margin'].min()):.4g}: oracle bit-identical ({sum(k.endswith('/l2') for k in res)} taps)")
        flat["case_names"] = np.array([t[0] for t in table])
        flat["case_table"] = np.array([t[1:] for t in table], dtype=np.int64)       # B, T, clip seed, bandwidth_id
        out = os.path.join(HERE, f"arch_{name}.npz")
        np.savez_compressed(out, **flat)
        size = os.path.getsize(out)
        assert size < MAX_FILE, (out, size)
        total += size
        print(f"{name}: {out} {size} bytes")
        del ref, orc, o64, sd
    assert total < MAX_TOTAL, total
    print("fixtures written to", HERE, total, "bytes in all")


if __name__ == "__main__":
    main()
