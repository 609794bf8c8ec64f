"""The architecture variants of tests/golden/arch_<name>.npz (tests/golden/make_golden_archs.py wrote them from the real
reference): the architecture and case table of each fixture, its regenerated weights and clips, and the oracle's run of a
case, computed once and shared by tests/test_arch_variants.py and tests/test_arch_variants_host.py."""
import functools
import json
import os

import numpy as np
import torch

from tests.util import GOLDEN, manifest

VARIANTS = ("narrow", "mid16", "last16", "wide")
CASES = ("small", "rows")


@functools.lru_cache(maxsize=None)
def variant(name: str):
    """(ArchConfig, {case: (B, T, clip seed, bandwidth_id)}, the opened fixture)."""
    from wavtokenizer_amd.config import ArchConfig
    g = np.load(os.path.join(GOLDEN, f"arch_{name}.npz"))
    d = json.loads(str(g["arch"]))
    d["ratios"], d["bandwidths"] = tuple(d["ratios"]), tuple(d["bandwidths"])
    cases = {str(c): tuple(int(v) for v in row) for c, row in zip(g["case_names"], g["case_table"])}
    return ArchConfig(**d), cases, g


@functools.lru_cache(maxsize=2)
def state_dict(name: str):
    from wavtokenizer_amd import synth
    return synth.make_state_dict(variant(name)[0], seed=manifest()["weight_seed"])


def clips(name: str, case: str) -> np.ndarray:
    from wavtokenizer_amd import synth
    B, T, seed, _bw = variant(name)[1][case]
    return synth.make_clips(B, T, seed)


def oracle(name: str, float64: bool = False):
    from oracle.cpu_ref import OracleWavTokenizer
    sd = state_dict(name)
    return OracleWavTokenizer(variant(name)[0], {k: torch.from_numpy(v).double() for k, v in sd.items()} if float64 else sd)


@functools.lru_cache(maxsize=2)
def oracle_run(name: str, case: str):
    """The fp32 oracle (= the reference, bit for bit where the fixture was written) on a case: features, codes, waveform, taps.
    Read-only: shared between tests."""
    bw = torch.tensor([variant(name)[1][case][3]])
    taps = {}
    with torch.inference_mode():
        wav = torch.from_numpy(clips(name, case))
        feats, codes = oracle(name).encode_infer(wav, bw, taps)
        out = oracle(name).decode(feats, bw, taps)
    return {"feats": feats, "codes": codes, "wav": out, "taps": taps}


@functools.lru_cache(maxsize=2)
def oracle64_run(name: str, case: str):
    """The same op sequence in float64 (weights and inputs cast up): pre-VQ embedding, codes, and the waveform decoded from the
    FP32 oracle's features (the same features on every side of a comparison)."""
    bw = torch.tensor([variant(name)[1][case][3]])
    o64 = oracle(name, float64=True)
    taps = {}
    with torch.inference_mode():
        _f, codes = o64.encode_infer(torch.from_numpy(clips(name, case)).double(), bw, taps)
        out = o64.decode(oracle_run(name, case)["feats"].double(), bw)
    emb_key = max((k for k in taps if k.startswith("enc.")), key=lambda k: int(k.split(".")[1]))      # last encoder tap
    return {"emb_key": emb_key, "emb": taps[emb_key], "codes": codes, "wav": out, "margin": taps["vq.margin"]}
