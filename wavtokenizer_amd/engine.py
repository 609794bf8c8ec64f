"""The native side of a ``WavTokenizer``: the wt_model handle with its cached plans, workspaces and staging buffers, and the
small helpers that pass tensors, streams and status words across the C ABI."""
from __future__ import annotations

import ctypes
import os
from typing import Any, Dict, List, Tuple

import numpy as np
import torch

from . import _capi
from ._capi import WtArch, WtTensor, _ptr, _stream as _stream_ptr, check, lib  # noqa: F401  (_ptr, _stream_ptr: re-exported)
from .config import ArchConfig


# --------------------------------------------------------------------------------- engine
class _Engine:
    """Owns the wt_model handle, the (kind, B, len) plans and their workspaces."""

    def __init__(self):
        self.model = ctypes.c_void_p()
        # cached plans (+ workspaces): least recently used ones go first once there are more than max_plans of them or
        # their workspaces exceed max_ws_bytes (a file-by-file caller meets a new length, hence a new plan, per file)
        self.max_plans = int(os.environ.get("WAVTOK_MAX_PLANS", "64"))
        self.max_ws_bytes = int(float(os.environ.get("WAVTOK_MAX_WORKSPACE_GB", "16")) * (1 << 30))
        # plans are per HIP stream (a plan owns a workspace): at most this many non-default streams keep plans at a time; a
        # caller that makes a new stream (or takes one of torch's 32 pooled side streams) per request would otherwise fill the
        # LRU with plans + workspaces + recorded graphs of streams it never uses again (the least recently used stream goes first)
        self.max_streams = int(os.environ.get("WAVTOK_MAX_STREAMS", "4"))
        self.stream_lru: List[int] = []
        self.plans: Dict[tuple, Tuple[ctypes.c_void_p, torch.Tensor]] = {}
        self.io: Dict[int, tuple] = {}     # staging buffers of graph plans by plan handle: (inputs, outputs) of WavTokenizer._call
        self.device_index = -1
        self._keepalive: List[Any] = []

    def close(self):
        for plan, _ws in self.plans.values():
            lib.wt_plan_destroy(plan)
        self.plans.clear()
        self.io.clear()
        if self.model:
            lib.wt_model_destroy(self.model)
            self.model = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, arch: ArchConfig, state: Dict[str, torch.Tensor], device_index: int):
        self.close()
        wa = WtArch()
        wa.n_ratios = len(arch.ratios)
        for i, r in enumerate(arch.ratios):
            wa.ratios[i] = int(r)
        wa.vq_bins, wa.num_quantizers, wa.input_channels = arch.vq_bins, arch.num_quantizers, arch.input_channels
        wa.dim, wa.intermediate_dim, wa.num_layers = arch.dim, arch.intermediate_dim, arch.num_layers
        wa.adanorm_num_embeddings = arch.adanorm_num_embeddings
        wa.n_fft, wa.hop_length = arch.n_fft, arch.hop_length
        wa.padding_same = 1 if arch.padding == "same" else 0
        arrs = []
        tens = (WtTensor * len(state))()
        for i, (k, v) in enumerate(state.items()):
            a = np.ascontiguousarray(v.detach().to("cpu", torch.float32).numpy())
            arrs.append(a)
            tens[i].name = k.encode()
            tens[i].data = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            tens[i].numel = a.size
        check(lib.wt_model_create(ctypes.byref(wa), tens, len(state), device_index, ctypes.byref(self.model)),
              "wt_model_create")
        self.device_index = device_index

    def load_packed(self, image: np.ndarray, device_index: int):
        """Upload a packed image (WavTokenizer.save_packed): nothing is folded, packed or split again."""
        self.close()
        check(lib.wt_model_create_packed(image.ctypes.data_as(ctypes.c_void_p), image.nbytes, device_index,
                                         ctypes.byref(self.model)), "wt_model_create_packed")
        self.device_index = device_index

    def export(self) -> np.ndarray:
        n = lib.wt_model_export_bytes(self.model)
        buf = np.empty(n, dtype=np.uint8)
        check(lib.wt_model_export(self.model, buf.ctypes.data_as(ctypes.c_void_p), n), "wt_model_export")
        used = lib.wt_packed_bytes(buf.ctypes.data_as(ctypes.c_void_p), n)       # wt_model_export_bytes is an upper bound
        return buf[:used] if 0 < used <= n else buf

    @staticmethod
    def _key(kind: int, B: int, length: int, flags: int, device, sites: int = 0) -> tuple:
        """A plan owns a workspace, so it serves ONE stream: calls made under another current stream than the default one
        get plans (and staging buffers) of their own, keyed (..., stream handle).  Two streams can then run the same model
        side by side (sharding.StepRunner(lanes=2)); the library orders their persistent LSTM launches itself (run.cpp).
        Key: (kind, B, length, flags) on the default stream, + (stream,) on another one, + (stream, fp32 site mask) for a
        plan with range sites on fp32 operands (stream 0 = the default stream)."""
        sp = torch.cuda.current_stream(device).cuda_stream if device is not None else 0
        if sites:
            return (kind, B, length, flags, sp, sites)
        return (kind, B, length, flags) if not sp else (kind, B, length, flags, sp)

    def _touch_stream(self, sp: int):
        if not sp:
            return
        if sp in self.stream_lru:
            self.stream_lru.remove(sp)
        self.stream_lru.append(sp)
        while len(self.stream_lru) > self.max_streams:
            old = self.stream_lru.pop(0)
            self.drop(lambda k: len(k) >= 5 and k[4] == old)

    def plan(self, kind: int, B: int, length: int, flags: int, device: torch.device, sites: int = 0):
        key = self._key(kind, B, length, flags, device, sites)
        hit = self.plans.pop(key, None)
        if hit is not None:
            self.plans[key] = hit                     # most recently used last (dicts keep insertion order)
            return hit
        if len(key) >= 5:
            self._touch_stream(key[4])
        p = ctypes.c_void_p()
        check(lib.wt_plan_create_ex(self.model, kind, B, length, flags, sites, ctypes.byref(p)), "wt_plan_create")
        need = lib.wt_plan_workspace_bytes(p)
        while self.plans and (len(self.plans) >= self.max_plans or
                              sum(w.numel() for _p, w in self.plans.values()) + need > self.max_ws_bytes):
            old = self.plans.pop(next(iter(self.plans)))[0]      # LRU: the least recently used plan + workspace
            lib.wt_plan_destroy(old)
            self.io.pop(old.value, None)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        self.plans[key] = (p, ws)
        return p, ws

    def drop(self, pred):
        """Destroys the cached plans (and their workspaces) whose key (kind, B, length, flags) satisfies pred."""
        for k in [k for k in self.plans if pred(k)]:
            plan = self.plans.pop(k)[0]
            lib.wt_plan_destroy(plan)
            self.io.pop(plan.value, None)


def site_name(site: int) -> str:
    """Range site (include/wavtokenizer_amd.h wt_range_site) -> the reference module it covers."""
    names = {_capi.WT_SITE_ENCODER: "feature_extractor.encodec.encoder + quantizer", _capi.WT_SITE_BB_EMBED: "backbone.embed",
             _capi.WT_SITE_RES0: "backbone.pos_net.0", _capi.WT_SITE_RES1: "backbone.pos_net.1", _capi.WT_SITE_ATTN: "backbone.pos_net.2",
             _capi.WT_SITE_RES2: "backbone.pos_net.3", _capi.WT_SITE_RES3: "backbone.pos_net.4", _capi.WT_SITE_HEAD: "backbone.final_layer_norm + head",
             _capi.WT_SITE_SEANET_DECODER: "feature_extractor.encodec.decoder"}
    if _capi.WT_SITE_CNX0 <= site < _capi.WT_SITE_HEAD:
        return "backbone.convnext.%d" % (site - _capi.WT_SITE_CNX0)
    return names.get(site, "site %d" % site)


def _fill(src, buf: torch.Tensor) -> torch.Tensor:
    """Writes one input of WavTokenizer._call into buf: a tensor is copied, a (shape, dtype, fill) input runs fill(buf)."""
    if isinstance(src, torch.Tensor):
        buf.copy_(src)
    else:
        src[2](buf)
    return buf


def _take_status(read, handle) -> int:
    """Reads and clears a status word: read is lib.wt_plan_status (handle: a plan) or lib.wt_model_status (the model)."""
    bits = ctypes.c_int32()
    check(read(handle, ctypes.byref(bits), 1), read.__name__)
    return bits.value
