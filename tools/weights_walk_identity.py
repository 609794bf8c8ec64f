#!/usr/bin/env python3
"""What the loaded library makes of the four test models (hop600, hop320, hop600 + SEANetDecoder, hop600 with three codebooks):
the sha256 of export(), the entry count and a sha256 over the whole wt_model_weight_info listing in order (every field but the
`data` addresses), for the model made from the state dict and for the one made from its own image.  Run it once per
library (WAVTOK_HIP_LIB=tools/lib/libwavtok_hip_prev.so for the parent's, tools/build_prev.sh) and compare the lines.

  --save DIR   also write each image to DIR/<variant>.wtpk
  --load DIR   also load DIR/<variant>.wtpk (written by the other library) and print the same figures for that model"""
import argparse
import ctypes
import dataclasses
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from wavtokenizer_amd import NAMED_ARCHS, _capi, synth
from wavtokenizer_amd.pretrained import _Engine

FIELDS = ("format", "name", "of", "numel", "ndim", "tap_pair", "acc_scale", "lazy_scale", "lazy", "archived", "alloc")


def variants():
    h6 = NAMED_ARCHS["hop600"]
    yield "hop600", h6, synth.make_state_dict(h6, seed=0)
    yield "hop320", NAMED_ARCHS["hop320"], synth.make_state_dict(NAMED_ARCHS["hop320"], seed=0)
    yield "hop600+seanet", h6, synth.make_state_dict(h6, seed=0, with_seanet_decoder=True)
    x3 = dataclasses.replace(h6, num_quantizers=3)
    yield "hop600x3", x3, synth.make_state_dict(x3, seed=0)


def figures(eng):
    """(sha256 of the image, entries, sha256 of the listing, the image)"""
    lib = _capi.lib
    h = hashlib.sha256()
    n = lib.wt_model_weight_count(eng.model)
    for i in range(n):
        w = _capi.WtWeightInfo(size=ctypes.sizeof(_capi.WtWeightInfo))
        _capi.check(lib.wt_model_weight_info(eng.model, i, ctypes.byref(w)), "wt_model_weight_info")
        h.update(repr([getattr(w, f) for f in FIELDS] + list(w.dims)).encode())
    image = eng.export()
    return hashlib.sha256(image.tobytes()).hexdigest(), n, h.hexdigest(), image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save")
    ap.add_argument("--load")
    args = ap.parse_args()
    print("library:", _capi.LIB_PATH, _capi.lib.wt_version().decode())
    dev = torch.cuda.current_device()
    for name, arch, sd in variants():
        state = {k: torch.from_numpy(v) for k, v in sd.items()}
        eng = _Engine()               # (the engine itself: the module tree of WavTokenizer drops the SEANetDecoder's tensors)
        eng.load(arch, state, dev)
        sha, n, listing, image = figures(eng)
        pk = _Engine()
        pk.load_packed(image, dev)
        psha, pn, plisting, _ = figures(pk)
        print(f"{name}: image sha256 {sha} ({image.nbytes} bytes), {n} entries, listing sha256 {listing}; "
              f"its packed model: image {'same' if psha == sha else psha}, {pn} entries, listing {'same' if plisting == listing else plisting}")
        pk.close()
        if args.save:
            os.makedirs(args.save, exist_ok=True)
            image.tofile(os.path.join(args.save, name + ".wtpk"))
        if args.load:
            other = np.fromfile(os.path.join(args.load, name + ".wtpk"), dtype=np.uint8)
            ot = _Engine()
            ot.load_packed(other, dev)
            osha, on, olisting, _ = figures(ot)
            print(f"{name}: loaded from {args.load}: image sha256 {osha}, {on} entries, listing sha256 {olisting}")
            ot.close()
        eng.close()


if __name__ == "__main__":
    main()
