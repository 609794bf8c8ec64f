"""Drop-in ``WavTokenizer`` (mirror of the reference's decoder/pretrained.py:32-239).

Same constructor classmethods, method names, argument meaning, tensor layouts and error
behaviour as the reference class; underneath, every method enqueues hand-written HIP kernels
through the C-ABI library (``include/wavtokenizer_amd.h``).  PyTorch supplies device memory,
the current HIP stream and the ``nn.Module`` parameter container (so ``state_dict()`` /
``load_state_dict()`` / ``.to(device)`` keep working with reference checkpoints) — no torch op
runs on the compute path, and there is no CPU fallback: calling a method while the module sits
on the CPU raises.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import Any, Dict, List, Optional

import numpy as np
import torch
import yaml
from torch import nn

from . import _capi
from ._capi import WavTokError, WtArch, check, lib
from .batched import _BatchedCalls, _ClipSpec, _OffRoute, _PcmSpec  # noqa: F401  (re-exported)
from .config import ArchConfig, arch_from_yaml_dict
from .engine import _Engine, _fill, _ptr, _stream_ptr, _take_status, site_name  # noqa: F401  (re-exported)
from .tree import (EncodecFeatures, EncodecModel, ISTFTHead, ResidualVectorQuantizer, SEANetDecoder,  # noqa: F401  (re-exported)
                   SEANetEncoder, VocosBackbone, _build_tree, _CodebookLayer, _Holder)


def _decode_codes_mixed_entry(plan, codes, lengths, K, bw, wav, ws, stream):
    """lib.wt_decode_codes_mixed in the argument order of WavTokenizer._call (inputs, scalars, outputs)."""
    return lib.wt_decode_codes_mixed(plan, codes, K, lengths, bw, wav, ws, stream)


# ------------------------------------------------------------------------------ public class
class WavTokenizer(_BatchedCalls, nn.Module):
    """Same surface as the reference class (decoder/pretrained.py:32); the calls that take many clips at once are
    batched._BatchedCalls'."""

    def __init__(self, feature_extractor: EncodecFeatures, backbone: VocosBackbone, head: ISTFTHead,
                 arch: Optional[ArchConfig] = None):
        super().__init__()
        self.feature_extractor = feature_extractor
        self.backbone = backbone
        self.head = head
        self._arch = arch
        self._engine = _Engine()
        self._dirty = True
        self._plan_flags = 0
        self._f16_gemm = False               # set_gemm_precision("f16"): the decode plan kinds alone get WT_PLAN_FLAG_F16_GEMM (_decode_flags)
        self._fp32_sites = 0                 # range sites (_capi.WT_SITE_*) that have left the split-f16 form after an overflow
        # strict status: None (default) = automatic: calls of up to _graph_max_clips clips (graph-replayed, bound by the host
        # anyway: the reference's own file-by-file usage) synchronise, check and REPEAT a failed call on the fallback path, so
        # an infer.py-style caller is never handed poisoned tensors; larger batches stay asynchronous and report on the next
        # call.  WAVTOK_STRICT_STATUS=1 / 0 or set_strict_status force it on / off for every size
        env_strict = os.environ.get("WAVTOK_STRICT_STATUS")
        self._strict = None if env_strict is None else env_strict == "1"
        # codes_to_features and indices outside the codebook (F.embedding raises IndexError, pretrained.py:236): "sync"
        # (default) synchronises after the gather (a few microseconds of work) and raises for the offending call, like the
        # reference on the CPU; "deferred" (opt-in, for pipelines that must not synchronise) raises on the NEXT call on this
        # model or in check_status(); "off" never looks.  The gathered features of a bad index are NaN in every mode.
        env_cc = os.environ.get("WAVTOK_CHECK_CODES", "sync")
        env_cc = {"1": "sync", "0": "off"}.get(env_cc, env_cc)
        if env_cc not in ("sync", "deferred", "off"):
            raise ValueError(f"WAVTOK_CHECK_CODES={env_cc!r}: use sync (or 1), deferred or off (or 0)")
        self._check_codes = env_cc
        self._bw_cache = None                # (tensor ref, version, index): bandwidth_id tensors living on the GPU
        self.fallback_events: List[str] = []   # device-side failures this model has answered by falling back (check_status reports them)
        # batches up to this many clips are replayed as one hipGraph per (shape) plan: they are bound by the host's
        # launch rate (about 100 launches per call), not by the GPU; 0 turns graphs off
        self._graph_max_clips = int(os.environ.get("WAVTOK_GRAPH_MAX_CLIPS", "16"))
        # encode_codes_many: two pinned host buffers that take turns carrying a group's CPU clips (and its lengths and code
        # offsets) to the GPU in one copy; the event behind a buffer's last upload guards it against reuse
        self._pin_bufs: List[Optional[torch.Tensor]] = [None, None]
        self._pin_events: List[Any] = [None, None]
        self._pin_next = 0
        self._emit_ws: Optional[torch.Tensor] = None      # decode_pcm / decode_pcm_many: the workspace of wt_emit launches of up to 64 clips
        # encode_codes_segmented_many: uniform batches of full segments on the mixed-length plan instead of the plain one (the same
        # bits; tools/segmented_bench.py case (d) measures both, the plain plan is not slower)
        self._segment_uniform_mixed = False
        for m in (feature_extractor, backbone, head):
            m._bind(self)

    # -- construction (pretrained.py:46-156) ---------------------------------------------------
    @classmethod
    def _from_config_node(cls, node: Dict[str, Any]) -> "WavTokenizer":
        arch = arch_from_yaml_dict({"model": {"init_args": node}})
        fe, bb, hd = _build_tree(arch)
        return cls(feature_extractor=fe, backbone=bb, head=hd, arch=arch)

    @classmethod
    def from_arch(cls, arch: ArchConfig) -> "WavTokenizer":
        fe, bb, hd = _build_tree(arch)
        return cls(feature_extractor=fe, backbone=bb, head=hd, arch=arch)

    @classmethod
    def from_hparams(cls, config_path: str) -> "WavTokenizer":
        with open(config_path, "r") as f:
            config = yaml.safe_load(f)
        return cls._from_config_node(config)

    @classmethod
    def from_hparams0802(cls, config_path: str) -> "WavTokenizer":
        with open(config_path, "r") as f:
            config = yaml.safe_load(f)
        return cls._from_config_node(config["model"]["init_args"])

    @staticmethod
    def _filter_state(state_dict_raw: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        # pretrained.py:103-105: drops the discriminators of the Lightning checkpoint
        return {k: v for k, v in state_dict_raw.items()
                if k.startswith("backbone.") or k.startswith("head.") or k.startswith("feature_extractor.")}

    @staticmethod
    def _read_ckpt(model_path: str) -> Dict[str, torch.Tensor]:
        # Lightning .ckpt: a pickle; only tensors are read (weights_only), nothing else is executed
        return torch.load(model_path, map_location="cpu", weights_only=True)["state_dict"]

    @classmethod
    def from_pretrained0802(cls, config_path: str, model_path: str) -> "WavTokenizer":
        model = cls.from_hparams0802(config_path)
        model.load_state_dict(cls._filter_state(cls._read_ckpt(model_path)))
        model.eval()
        return model

    @staticmethod
    def _best_checkpoints(folder: str, keep: int = 3) -> List[str]:
        """File names of the `vocos_*` checkpoints to average: the reference ranks them by the six characters that
        precede the extension (the validation loss printed into the name) as STRINGS and keeps every file whose tag is
        among the `keep` smallest, in directory order (pretrained.py:122-138)."""
        names = [n for n in os.listdir(folder) if n.startswith("vocos_")]
        loss_tag = lambda n: n[-11:-5]
        chosen = set(sorted(loss_tag(n) for n in names)[:keep])
        return [n for n in names if loss_tag(n) in chosen]

    @classmethod
    def from_pretrained0911(cls, config_path: str, model_folder_path: str) -> "WavTokenizer":
        """Mean of the best `vocos_*` checkpoints of a folder (pretrained.py:117-156): tensors are summed in directory
        order and divided by the count, in their own dtype, exactly as the reference does."""
        model = cls.from_hparams0802(config_path)
        parts = [cls._filter_state(cls._read_ckpt(os.path.join(model_folder_path, n)))
                 for n in cls._best_checkpoints(model_folder_path)]
        if not parts:
            raise FileNotFoundError(f"no vocos_* checkpoint in {model_folder_path}")
        mean_state = {}
        for key, first in parts[0].items():
            total = first.clone()
            for other in parts[1:]:
                total += other[key]
            mean_state[key] = total / len(parts)
        model.load_state_dict(mean_state)
        model.eval()
        return model

    # -- hot-path state: one pickle-free file holding exactly the hot-path tensors ------------------------------------
    def save_hot_state(self, path: str) -> None:
        """Write the hot-path state (the 289 reference keys this class keeps; discriminators, optimizer state and
        the rest of a Lightning checkpoint are gone) as one safetensors file: nothing is executed when it is read
        back, and it loads without unpickling a multi-GB training checkpoint."""
        from safetensors.torch import save_file
        sd = {k: v.detach().to("cpu", copy=True).contiguous() for k, v in self.state_dict().items()}
        save_file(sd, path, metadata={"format": "wavtokenizer_amd.hot_state.v1", "hop": str(self._arch.hop)})

    @classmethod
    def from_hot_state(cls, config_path: str, path: str) -> "WavTokenizer":
        """Counterpart of from_pretrained0802 (pretrained.py:95-114) for a file written by save_hot_state."""
        from safetensors.torch import load_file
        model = cls.from_hparams0802(config_path)
        model.load_state_dict(load_file(path, device="cpu"))
        model.eval()
        return model

    # -- packed image: what sits in HBM after loading, ready to upload again ------------------------------
    def save_packed(self, path: str) -> None:
        """Write the model as it sits in HBM (folded conv weights in [Cout][tap][Cin], LSTM lane packings, the packed
        ISTFT head and inverse-DFT basis, the S32 split copies and their scales) behind a header with a layout
        version and an architecture hash.  from_packed uploads it without folding, packing or splitting anything again.
        The model must be on the GPU (the image is read back from there)."""
        self._ensure_engine()
        self._engine.export().tofile(path)

    @classmethod
    def from_packed(cls, config_path: str, packed_path: str, device="cuda") -> "WavTokenizer":
        """Counterpart of from_pretrained0802 (pretrained.py:95-114) for a file written by save_packed: the file is
        memory-mapped and uploaded as it is.  The returned model keeps no copy of the reference's raw tensors (its
        nn.Module parameters are placeholders): state_dict() raises, load_state_dict() turns it into a normal model."""
        model = cls.from_hparams0802(config_path)
        image = np.memmap(packed_path, dtype=np.uint8, mode="r")
        wa, ver, ah = WtArch(), ctypes.c_int32(), ctypes.c_uint64()
        check(lib.wt_packed_info(image.ctypes.data_as(ctypes.c_void_p), image.nbytes, ctypes.byref(wa), ctypes.byref(ver),
                                 ctypes.byref(ah)), "wt_packed_info")
        a = model._arch
        # every field of wt_arch: the library sizes its launches from the image's architecture while this class sizes the
        # tensors it hands over from the config's (a 'same' image under a 'center' config would be written B*hop floats
        # past the end of the waveform tensor), so any difference is an error
        mine = {"ratios": tuple(a.ratios), "vq_bins": a.vq_bins, "num_quantizers": a.num_quantizers,
                "input_channels": a.input_channels, "dim": a.dim, "intermediate_dim": a.intermediate_dim,
                "num_layers": a.num_layers, "adanorm_num_embeddings": a.adanorm_num_embeddings, "n_fft": a.n_fft,
                "hop_length": a.hop_length, "padding": a.padding}
        theirs = {"ratios": tuple(wa.ratios[i] for i in range(wa.n_ratios)), "vq_bins": wa.vq_bins,
                  "num_quantizers": wa.num_quantizers, "input_channels": wa.input_channels, "dim": wa.dim,
                  "intermediate_dim": wa.intermediate_dim, "num_layers": wa.num_layers,
                  "adanorm_num_embeddings": wa.adanorm_num_embeddings, "n_fft": wa.n_fft, "hop_length": wa.hop_length,
                  "padding": "same" if wa.padding_same else "center"}
        diff = {k: (theirs[k], mine[k]) for k in mine if mine[k] != theirs[k]}
        if diff:
            raise ValueError(f"packed file was written for another architecture (field: (file, config)): {diff}")
        dev = torch.device(device)
        model.eval()
        model = model.to(dev)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        model._engine.load_packed(np.asarray(image), idx)
        model._dirty = False
        model._packed_only = True
        return model

    def state_dict(self, *a, **kw):
        if getattr(self, "_packed_only", False):
            raise RuntimeError("this model was loaded from a packed image (from_packed): it holds the folded and packed "
                               "weights in HBM, not the reference's raw tensors; load a checkpoint to get a state_dict")
        return super().state_dict(*a, **kw)

    @classmethod
    def from_pretrained(cls, repo_id: str) -> "WavTokenizer":
        from huggingface_hub import hf_hub_download
        config_path = hf_hub_download(repo_id=repo_id, filename="config.yaml")
        model_path = hf_hub_download(repo_id=repo_id, filename="pytorch_model.bin")
        model = cls.from_hparams(config_path)
        state_dict = torch.load(model_path, map_location="cpu", weights_only=True)
        model.load_state_dict(state_dict, strict=False)
        model.eval()
        return model

    # -- nn.Module protocol: any weight or device change invalidates the packed HBM copy -------
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._dirty = True
        self._packed_only = False
        return out

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        if not getattr(self, "_packed_only", False):      # a packed model has nothing to re-pack from
            self._dirty = True
        return out

    def refresh_weights(self):
        """Call after mutating parameters in place."""
        self._dirty = True

    def set_debug_keep_stages(self, on: bool, unfused: bool = False):
        """Parity tests: keep every stage buffer of the next plans distinct in the workspace (and snapshot the in-place
        residual stream).  The kernels stay the shipped ones; `unfused=True` selects the unfused debug twin instead
        (raw fp32 tensors between stages)."""
        f = self._plan_flags & ~(_capi.WT_PLAN_FLAG_KEEP_STAGES | _capi.WT_PLAN_FLAG_UNFUSED)
        if on:
            f |= _capi.WT_PLAN_FLAG_KEEP_STAGES | (_capi.WT_PLAN_FLAG_UNFUSED if unfused else 0)
        self._plan_flags = f

    def set_strict_status(self, on: bool):
        """Device-side failures of a call (an activation beyond the f16 range of the split-f16 form; a persistent-LSTM step
        barrier that timed out) always overwrite that call's outputs (codes = -1, NaN) and surface as an error on the
        NEXT call on this model, whatever its shape (the library keeps one host-mapped status word per model beside the
        per-plan ones), which this class answers by falling back for good (fp32 GEMMs / launch-per-step LSTM for every
        plan of the model) and running that next call.  strict=True additionally synchronises after every call, checks, falls back and REPEATS
        the failed call itself, so no poisoned result is ever handed out (costs the host/GPU overlap between calls).
        Default (None): strict for calls of up to the graph batch limit (16 clips), asynchronous above."""
        self._strict = None if on is None else bool(on)

    def _is_strict(self, B: int) -> bool:
        if self._strict is None:
            return 0 < B <= self._graph_max_clips
        return self._strict

    def check_status(self):
        """Synchronise and raise WavTokError if any call since the last check failed on the device: failures still pending
        in the status words, and failures that a later call has already consumed and answered by falling back
        (self.fallback_events; in non-strict mode the failed call's poisoned outputs were handed out)."""
        dev = self._device()
        torch.cuda.current_stream(dev).synchronize()
        # the model's word first: it is what decides (every plan's guard step reports into it, and it outlives plans the
        # LRU has destroyed); the plans' own words only say which plans reported since the last check and may hold
        # failures that a later call has already consumed and answered by falling back
        mbits = _take_status(lib.wt_model_status, self._engine.model) if self._engine.model else 0
        seen = []
        for key, (plan, _ws) in self._engine.plans.items():
            bits = _take_status(lib.wt_plan_status, plan)
            if bits:
                seen.append((key, bits))
        if mbits & _capi.WT_STATUS_BIT_RANGE:
            self._answer_range()
        bad = (seen or [("model", mbits)]) if mbits else []
        events, self.fallback_events = self.fallback_events, []
        if events and not bad:
            raise WavTokError("device-side failures since the last check, already answered by a fallback: %s" % events)
        self._poll_bad_codes()
        if bad:
            raise WavTokError("device-side failure in earlier calls (plan key, status bits): %s; their outputs were "
                              "overwritten with -1 / NaN; later calls fall back (fp32 operands at the reporting site / step LSTM)" % bad)

    def _answer_range(self) -> str:
        """An S32 producer met |v| >= 65504.  The plans know which range sites reported (wt_plan_range_sites): the LOWEST
        one that is still on split-f16 operands goes to fp32 operands (its GEMMs then run on the fp32 MFMA chain; sites
        behind it usually report as well, because infinities propagate, and are left alone until they report on their
        own).  Without attribution (the plan is gone) the whole model falls back, as in round 3."""
        mask = 0
        for plan, _ws in self._engine.plans.values():
            m = ctypes.c_uint64()
            check(lib.wt_plan_range_sites(plan, ctypes.byref(m), 1), "wt_plan_range_sites")
            mask |= m.value
        new = mask & ~self._fp32_sites
        if new:
            site = (new & -new).bit_length() - 1
            self._fp32_sites |= 1 << site
            return "range site %d (%s) now keeps fp32 operands" % (site, site_name(site))
        self._plan_flags |= _capi.WT_PLAN_FLAG_FP32_GEMM
        self._f16_gemm = False
        return "no site attribution left: the whole model now runs fp32 GEMMs"

    def set_gemm_precision(self, mode: str):
        """"f16x3" (default): dense layers on the fp32-equivalent split-f16 MFMA kernel; "f32": the plain
        fp32 MFMA chain everywhere.  Both accumulate in fp32; measured error vs float64 is lower for f16x3.
        "f16": half-precision inference for the decoder, for callers that hold codes and want audio: decode, decode_many,
        decode_codes, decode_codes_many, model(wav) and model.backbone(...) multiply the f16 hi halves of the split-f16 operands
        alone (one MFMA per product instead of three, fp32 accumulate; waveform error near 1e-3 relative instead of 1e-5).
        The encoder, the VQ and the codes, codes_to_features, model.head(...), the SEANet callables and range_report stay on
        f16x3 whatever the mode."""
        if mode not in ("f16x3", "f32", "f16"):
            raise ValueError("mode must be 'f16x3', 'f32' or 'f16'")
        self._plan_flags = (self._plan_flags | _capi.WT_PLAN_FLAG_FP32_GEMM) if mode == "f32" else \
            (self._plan_flags & ~_capi.WT_PLAN_FLAG_FP32_GEMM)
        self._f16_gemm = mode == "f16"

    def _decode_flags(self, flags: int) -> int:
        """The flags of a decode-kind plan (WT_PLAN_DECODE, _MIXED, _CODES, _CODES_MIXED): `flags` plus the one-product GEMM mode
        where it is set and the plan runs split-f16 operands at all (the library refuses it beside FP32_GEMM or UNFUSED)."""
        if self._f16_gemm and not (flags & (_capi.WT_PLAN_FLAG_FP32_GEMM | _capi.WT_PLAN_FLAG_UNFUSED)):
            return flags | _capi.WT_PLAN_FLAG_F16_GEMM
        return flags

    def set_check_codes(self, mode: str):
        """How codes_to_features reports an index outside the codebook: "sync" (default: synchronise and raise for the
        offending call, like the reference), "deferred" (IndexError on the next call on this model or in check_status(), no
        stream synchronisation) or "off"."""
        if mode not in ("deferred", "sync", "off"):
            raise ValueError("mode must be 'deferred', 'sync' or 'off'")
        self._check_codes = mode

    @property
    def persistent_lstm(self) -> bool:
        """True while this model's plans may launch the persistent LSTM kernel (the library's own word: a 256-CU device and
        no lost-co-residency report so far)."""
        return bool(self._engine.model) and bool(lib.wt_model_persistent_lstm(self._engine.model))

    def _poll_bad_codes(self):
        if self._check_codes != "off" and self._engine.model and lib.wt_model_take_bad_codes(self._engine.model):
            raise IndexError("index out of range in self")

    def set_graph_max_clips(self, n: int):
        """Largest batch whose encode / decode plans are recorded and replayed as a hipGraph (default 16; 0 = never)."""
        self._graph_max_clips = int(n)

    def _graph_flags(self, B: int) -> int:
        if 0 < B <= self._graph_max_clips and not (self._plan_flags & _capi.WT_PLAN_FLAG_KEEP_STAGES):
            return self._plan_flags | _capi.WT_PLAN_FLAG_GRAPH
        return self._plan_flags

    def _guarded(self, dev: torch.device, call, strict: bool = False):
        """Runs call() -> (outputs, plan), one _call, with the fallbacks for device-side failures (set_strict_status) and
        returns the outputs.  call() plans from the CURRENT flags and fp32 sites, so a fallback that changes them re-plans."""
        for attempt in range(8):
            try:
                out, plan = call()
            except WavTokError as e:
                if e.status == _capi.WT_ERR_LSTM_SYNC and attempt < 7:
                    self.fallback_events.append("persistent LSTM lost co-residency in an earlier call (its outputs were poisoned): "
                                                "the model now runs the launch-per-step LSTM")
                    continue                                  # the model's plans now run the step LSTM
                if e.status == _capi.WT_ERR_RANGE and attempt < 7:
                    self.fallback_events.append("an earlier call left the f16 range of the split-f16 form (its outputs were "
                                                "poisoned): " + self._answer_range())
                    continue
                raise
            if not strict:
                return out
            torch.cuda.current_stream(dev).synchronize()
            bits = _take_status(lib.wt_plan_status, plan)
            if not bits:
                return out
            what = self._answer_range() if bits & _capi.WT_STATUS_BIT_RANGE else "launch-per-step LSTM"
            self.fallback_events.append("strict mode: the call failed on the device (status bits %d) and was repeated on the fallback path: %s" % (bits, what))
        raise WavTokError("the call kept failing on the device after the fp32 / step-LSTM fallbacks")

    def _sites(self, kind: int) -> int:
        """The fp32 range sites that matter to a plan kind (so that an overflow in the decoder does not re-plan the encoder)."""
        m = self._fp32_sites
        if kind in (_capi.WT_PLAN_ENCODE, _capi.WT_PLAN_UNIT_LSTM, _capi.WT_PLAN_QUANTIZE):
            return m & (1 << _capi.WT_SITE_ENCODER)
        if kind == _capi.WT_PLAN_HEAD:
            return m & (1 << _capi.WT_SITE_HEAD)
        if kind == _capi.WT_PLAN_SEANET_DECODER:
            return m & (1 << _capi.WT_SITE_SEANET_DECODER)
        # the decode kinds (WT_PLAN_DECODE, _MIXED, _CODES, _CODES_MIXED): every decoder site
        return m & ~((1 << _capi.WT_SITE_ENCODER) | (1 << _capi.WT_SITE_SEANET_DECODER))

    def range_report(self, audio_input: torch.Tensor, bandwidth_id=None) -> List[Dict[str, Any]]:
        """How far every split-f16 (S32) operand of the dense layers sits below the f16 limit on THIS input with THESE
        weights: one encode_infer + decode pass on plans created with WT_PLAN_FLAG_RANGE_REPORT (same kernels; behind every
        step the largest magnitude of each S32 buffer the step touches is measured).  Returns a list of
        {"plan", "step", "buffer", "amax", "headroom_bits" = log2(65504 / amax)} in execution order; an entry with
        amax = inf marks a tensor that left the range (the call's outputs are then poisoned, as always)."""
        import math
        dev = self._ensure_engine()
        bw = self._bandwidth_index(bandwidth_id if bandwidth_id is not None else torch.tensor([0]))
        audio = self._as_input(audio_input, dev)
        flags = (self._plan_flags | _capi.WT_PLAN_FLAG_RANGE_REPORT) & ~_capi.WT_PLAN_FLAG_GRAPH
        out: List[Dict[str, Any]] = []

        def collect(plan, what):
            i = 0
            step, buf, amax = ctypes.c_char_p(), ctypes.c_char_p(), ctypes.c_float()
            while lib.wt_plan_range_report(plan, i, ctypes.byref(step), ctypes.byref(buf), ctypes.byref(amax)) == 0:
                a = float(amax.value)
                out.append({"plan": what, "step": step.value.decode(), "buffer": buf.value.decode(), "amax": a,
                            "headroom_bits": (math.log2(65504.0 / a) if 0.0 < a < float("inf") else (float("inf") if a == 0.0 else float("-inf")))})
                i += 1

        (feats, _codes, _emb), pe = self._encode(*audio.shape, audio, flags, dev, want_emb=False)
        collect(pe, "encode")
        # the decoder is measured on the features the codes select (finite even if the encoder's own report shows an overflow)
        torch.cuda.current_stream(dev).synchronize()
        _take_status(lib.wt_plan_status, pe)
        _take_status(lib.wt_model_status, self._engine.model)
        fin = feats if torch.isfinite(feats).all() else torch.zeros_like(feats)
        _outs, pd = self._decode(fin, bw, flags, dev, want_backbone=False)
        collect(pd, "decode")
        torch.cuda.current_stream(dev).synchronize()
        _take_status(lib.wt_plan_status, pd)
        _take_status(lib.wt_model_status, self._engine.model)
        m = ctypes.c_uint64()
        for p in (pe, pd):
            check(lib.wt_plan_range_sites(p, ctypes.byref(m), 1), "wt_plan_range_sites")
        self._engine.drop(lambda k: k[3] & _capi.WT_PLAN_FLAG_RANGE_REPORT)
        return out

    def set_lstm_mode(self, mode: str):
        """"persistent" (default): the whole LSTM recurrence in one launch (per-XCD clip groups, weights resident);
        "step": one launch per time step."""
        if mode not in ("persistent", "step"):
            raise ValueError("mode must be 'persistent' or 'step'")
        self._plan_flags = (self._plan_flags | _capi.WT_PLAN_FLAG_STEP_LSTM) if mode == "step" else \
            (self._plan_flags & ~_capi.WT_PLAN_FLAG_STEP_LSTM)

    @property
    def arch(self) -> ArchConfig:
        return self._arch

    def _wave_len(self, L: int) -> int:
        """Samples per clip the ISTFT head returns for L frames (spectral_ops.py:43-47): 'same' L * hop, 'center' (L - 1) * hop."""
        return L * self._arch.hop_length if self._arch.padding == "same" else (L - 1) * self._arch.hop_length

    @property
    def hop_length(self) -> int:
        return self._arch.hop

    def _device(self) -> torch.device:
        return self.backbone.embed.weight.device

    def _ensure_engine(self) -> torch.device:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("wavtokenizer_amd runs only on an AMD GPU: move the model with .to('cuda'). "
                               "There is no CPU path in this package.")
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        if self._dirty or self._engine.device_index != idx:
            self._engine.load(self._arch, self.state_dict(), idx)
            self._dirty = False
        self._poll_bad_codes()          # an earlier codes_to_features met a bad index (deferred mode: found without a sync)
        return torch.device("cuda", idx)

    @staticmethod
    def _as_input(x: torch.Tensor, dev: torch.device, dtype=torch.float32) -> torch.Tensor:
        if x.device != dev:
            raise RuntimeError(f"input is on {x.device} but the model is on {dev}")
        return x.to(dtype).contiguous()

    # -- kernels ------------------------------------------------------------------------------------
    def _call(self, entry, kind: int, B: int, length: int, flags: int, dev: torch.device, ins, outs, scalars=(), name=None,
              borrow: bool = False):
        """One call of a C run entry point, entry(plan, inputs..., scalars..., outputs..., workspace, stream), on the plan
        (kind, B, length, flags) with the kind's fp32 sites.  ins: per input the tensor itself, or (shape, dtype, fill) for a
        buffer that fill(buffer) writes.  outs: per output (shape, dtype, wanted), or None for a null pointer; a direct call
        passes null for an unwanted output too.  name: what a failed call is reported as (default: entry's own name).
        borrow: a graph-replayed call hands out the plan's own staging buffers instead of copies; they hold the results until the
        next call on the plan (for a caller that consumes them on the same stream before it returns).
        Returns (outputs, None where not wanted; plan)."""
        plan, ws = self._engine.plan(kind, B, length, flags, dev, self._sites(kind))
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        graph = flags & _capi.WT_PLAN_FLAG_GRAPH
        if graph:
            # a recorded hipGraph replays fixed addresses: the plan keeps staging buffers, the inputs are copied in and the
            # results handed out as copies.  Every output buffer is passed, wanted or not: the recording is keyed by the
            # pointers (wt_plan::GraphKey), so encode_infer (no emb) and SEANetEncoder.forward (emb) alternating on one
            # plan would otherwise record it again on every call
            io = self._engine.io.get(plan.value)
            if io is None:
                io = self._engine.io[plan.value] = (
                    [new(x.shape, x.dtype) if isinstance(x, torch.Tensor) else new(*x[:2]) for x in ins],
                    [new(*o[:2]) if o is not None else None for o in outs])
            bufs, obufs = io
            for x, buf in zip(ins, bufs):
                _fill(x, buf)
        else:
            bufs = [x if isinstance(x, torch.Tensor) else _fill(x, new(*x[:2])) for x in ins]
            obufs = [new(*o[:2]) if o is not None and o[2] else None for o in outs]
        check(entry(plan, *map(_ptr, bufs), *scalars, *map(_ptr, obufs), _ptr(ws), _stream_ptr(dev)), name or entry.__name__)
        if graph:
            return tuple((b if borrow else b.clone()) if o is not None and o[2] else None for o, b in zip(outs, obufs)), plan
        return tuple(obufs), plan

    # -- staging layouts: the ONE place per plan kind that states its entry point, inputs, outputs and scalars.  A recorded graph is
    # keyed by the staging pointers (wt_plan::GraphKey): every caller of a plan comes through here and so stays on one recording
    def _encode(self, B: int, T: int, wav, flags: int, dev: torch.device, want_emb: bool, want_feats: bool = True):
        """WT_PLAN_ENCODE, plain: wav, a tensor (B, T) or the fill of one -> ((features, codes, emb), plan).  Without want_feats a
        direct call passes a null features pointer (the library then skips the gather); a graph plan keeps passing its staging
        buffer, so encode_infer, encode_codes and a uniform batch of segments share one recording."""
        L = self._arch.frames(T)
        wav = wav if isinstance(wav, torch.Tensor) else ((B, T), torch.float32, wav)
        return self._call(lib.wt_encode, _capi.WT_PLAN_ENCODE, B, T, flags, dev, (wav,),
                          (((B, 512, L), torch.float32, want_feats), ((1, B, L), torch.int64, True), ((B, 512, L), torch.float32, want_emb)),
                          name="wt_encode")

    def _encode_mixed(self, B: int, T_pad: int, fill_wav, lengths, dev: torch.device, want_feats: bool):
        """WT_PLAN_ENCODE with WT_PLAN_FLAG_MIXED_LENGTH: ((features [B, 512, L_pad], codes [1, B, L_pad], None: no emb), plan),
        -1 / 0 past each clip's frames; samples past a clip's length are never read.  want_feats as in _encode."""
        L = self._arch.frames(T_pad)
        return self._call(lib.wt_encode_mixed, _capi.WT_PLAN_ENCODE, B, T_pad, self._graph_flags(B) | _capi.WT_PLAN_FLAG_MIXED_LENGTH,
                          dev, (((B, T_pad), torch.float32, fill_wav), self._lengths_input(lengths)),
                          (((B, 512, L), torch.float32, want_feats), ((1, B, L), torch.int64, True), None), name="wt_encode_mixed")

    def _rvq_codes_out(self, n_q: int, B: int, L: int, flags: int):
        """The codes output of a residual VQ _call.  n_q is an argument of the call, not of the plan, while a graph plan keeps ONE
        staging buffer: it is sized for every codebook, [num_quantizers][B][L], and a call writes its first n_q slabs (the
        recording is keyed by n_q).  The caller takes [:n_q] of what _call returns."""
        nq = self._arch.num_quantizers if flags & _capi.WT_PLAN_FLAG_GRAPH else n_q
        return ((nq, B, L), torch.int64, True)

    def _encode_rvq(self, B: int, T: int, wav, n_q: int, flags: int, dev: torch.device):
        """WT_PLAN_ENCODE with WT_PLAN_FLAG_RVQ, plain: wav, a tensor (B, T) or the fill of one -> ((codes [n_q, B, L],), plan)."""
        L = self._arch.frames(T)
        wav = wav if isinstance(wav, torch.Tensor) else ((B, T), torch.float32, wav)
        flags |= _capi.WT_PLAN_FLAG_RVQ
        (codes,), plan = self._call(lib.wt_encode_rvq, _capi.WT_PLAN_ENCODE, B, T, flags, dev, (wav,),
                                    (self._rvq_codes_out(n_q, B, L, flags),), (n_q,), name="wt_encode_rvq")
        return (codes[:n_q],), plan

    def _encode_rvq_mixed(self, B: int, T_pad: int, fill_wav, lengths, n_q: int, dev: torch.device):
        """WT_PLAN_ENCODE with WT_PLAN_FLAG_RVQ | WT_PLAN_FLAG_MIXED_LENGTH: ((codes [n_q, B, L_pad],), plan), -1 past each clip's
        frames in every row; samples past a clip's length are never read."""
        L = self._arch.frames(T_pad)
        flags = self._graph_flags(B) | _capi.WT_PLAN_FLAG_MIXED_LENGTH | _capi.WT_PLAN_FLAG_RVQ
        (codes,), plan = self._call(lib.wt_encode_rvq_mixed, _capi.WT_PLAN_ENCODE, B, T_pad, flags, dev,
                                    (((B, T_pad), torch.float32, fill_wav), self._lengths_input(lengths)),
                                    (self._rvq_codes_out(n_q, B, L, flags),), (n_q,), name="wt_encode_rvq_mixed")
        return (codes[:n_q],), plan

    def _quantize(self, features: torch.Tensor, n_q: int, flags: int, dev: torch.device):
        """WT_PLAN_QUANTIZE: features (B, 512, L) fp32 -> ((codes [n_q, B, L],), plan)."""
        B, _, L = features.shape
        (codes,), plan = self._call(lib.wt_quantize, _capi.WT_PLAN_QUANTIZE, B, L, flags, dev, (features,),
                                    (self._rvq_codes_out(n_q, B, L, flags),), (n_q,))
        return (codes[:n_q],), plan

    def _check_n_q(self, who: str, n_q) -> int:
        """The number of residual VQ rounds of a call, checked before any GPU work."""
        if isinstance(n_q, bool) or not isinstance(n_q, (int, np.integer)):
            raise ValueError(who + ": n_q must be an int between 1 and the number of codebooks, or None")
        if not 1 <= int(n_q) <= self._arch.num_quantizers:
            raise WavTokError(who + ": n_q must be between 1 and the number of codebooks", _capi.WT_ERR_INVALID)
        return int(n_q)

    def _run_quantize(self, x: torch.Tensor, n_q: int) -> torch.Tensor:
        """quantizer.encode: features (B, 512, L) -> codes (n_q, B, L) on WT_PLAN_QUANTIZE."""
        n_q = self._check_n_q("quantizer.encode", n_q)
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != self.feature_extractor.encodec.quantizer.dimension:
            raise ValueError("quantizer.encode takes features (B, %d, L): the codebook width" % self.feature_extractor.encodec.quantizer.dimension)
        if x.shape[1] != self._arch.input_channels:
            raise WavTokError("residual VQ plans need input_channels and the encoder width equal to the codebook width", _capi.WT_ERR_INVALID)
        if x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError("quantizer.encode: empty features")
        dev = self._ensure_engine()
        x = self._as_input(x, dev)
        B = x.shape[0]
        return self._guarded(dev, lambda: self._quantize(x, n_q, self._graph_flags(B), dev), self._is_strict(B))[0]

    def _decode(self, features: torch.Tensor, bw: int, flags: int, dev: torch.device, want_backbone: bool):
        """WT_PLAN_DECODE: features (B, 512, L) -> ((waveform, backbone output), plan)."""
        B, _, L = features.shape
        # no backbone buffer at all unless asked for: a graph plan's staging has none
        bb = ((B, L, self._arch.dim), torch.float32, True) if want_backbone else None
        return self._call(lib.wt_decode, _capi.WT_PLAN_DECODE, B, L, flags, dev, (features,),
                          (((B, self._wave_len(L)), torch.float32, True), bb), (bw,))

    def _decode_mixed(self, B: int, L_pad: int, fill_feats, lengths, bw: int, dev: torch.device):
        """WT_PLAN_DECODE_MIXED: ((waveforms (B, wave_len(L_pad)),), plan), clip j's own samples first and zeros behind them;
        frames past a clip's length are read and dropped by the first kernel."""
        return self._call(lib.wt_decode_mixed, _capi.WT_PLAN_DECODE_MIXED, B, L_pad, self._decode_flags(self._graph_flags(B)), dev,
                          (((B, self._arch.input_channels, L_pad), torch.float32, fill_feats), self._lengths_input(lengths)),
                          (((B, self._wave_len(L_pad)), torch.float32, True),), (bw,))

    def _codes_staging(self, K: int, B: int, L: int, flags: int, fill):
        """The codes input of a decode-from-codes _call.  K is an argument of the call, not of the plan, while a graph plan
        keeps ONE staging buffer: it is sized for every codebook, [num_quantizers][B][L], and a call fills its first K slabs
        (they are the call's [K][B][L] array; the recording is keyed by K).  fill(buf[:K]) writes them."""
        nq = self._arch.num_quantizers if flags & _capi.WT_PLAN_FLAG_GRAPH else K
        return ((nq, B, L), torch.int64, lambda buf: fill(buf[:K]))

    def _decode_codes(self, codes: torch.Tensor, bw: int, flags: int, dev: torch.device, borrow: bool = False):
        """WT_PLAN_DECODE_CODES: codes (K, B, L) int64 -> ((waveform, None), plan)."""
        K, B, L = codes.shape
        graph = flags & _capi.WT_PLAN_FLAG_GRAPH
        ins = (self._codes_staging(K, B, L, flags, lambda buf: buf.copy_(codes)),) if graph else (codes,)
        return self._call(lib.wt_decode_codes, _capi.WT_PLAN_DECODE_CODES, B, L, flags, dev, ins,
                          (((B, self._wave_len(L)), torch.float32, True), None), (K, bw), borrow=borrow)

    def _decode_codes_mixed(self, K: int, B: int, L_pad: int, fill_codes, lengths, bw: int, dev: torch.device, borrow: bool = False):
        """WT_PLAN_DECODE_CODES_MIXED, the counterpart of _decode_mixed: fill_codes writes the (K, B, L_pad) codes; what they hold
        past a clip's frames is never read."""
        flags = self._decode_flags(self._graph_flags(B))
        return self._call(_decode_codes_mixed_entry, _capi.WT_PLAN_DECODE_CODES_MIXED, B, L_pad, flags, dev,
                          (self._codes_staging(K, B, L_pad, flags, fill_codes), self._lengths_input(lengths)),
                          (((B, self._wave_len(L_pad)), torch.float32, True),), (K, bw), name="wt_decode_codes_mixed", borrow=borrow)

    @staticmethod
    def _lengths_input(lengths):
        """The (B,) int32 lengths input of a mixed-length _call, from a Python list or from a tensor on the GPU."""
        src = lengths if isinstance(lengths, torch.Tensor) else torch.tensor(lengths, dtype=torch.int32)
        return ((len(lengths),), torch.int32, lambda buf: buf.copy_(src))

    def _run_encode(self, audio: torch.Tensor, want_emb: bool = True):
        dev = self._ensure_engine()
        assert audio.dim() == 2, "expected audio of shape (B, T)"
        audio = self._as_input(audio, dev)
        B, T = audio.shape
        return self._guarded(dev, lambda: self._encode(B, T, audio, self._graph_flags(B), dev, want_emb), self._is_strict(B))

    @torch.inference_mode()
    def encode_codes(self, audio_input: torch.Tensor, bandwidth_id=None, n_q: Optional[int] = None, normalize: Optional[str] = None,
                     target_db: float = 0.0, return_scales: bool = False, target_lufs: Optional[float] = None, *,
                     max_true_peak_db: Optional[float] = None):
        """encode_infer(audio_input, bandwidth_id=...)[1], the same bits, for a caller that wants the codes alone: (B, T) fp32 at
        the codec rate -> (1, B, L) int64.  A call that is not graph-replayed passes no feature buffer to the library (nothing
        gathers or writes the (B, 512, L) tensor); a graph-replayed one shares encode_infer's recording and staging buffers.
        Status, fallbacks and graphs behave as in encode_infer.
        n_q, an int in [1, num_quantizers]: residual VQ with the first n_q codebooks (the reference's quantizer.encode on the
        encoder output: nearest row of codebook k to the residual, subtract, next codebook) -> (n_q, B, L), on a plan of its own
        (WT_PLAN_FLAG_RVQ); the rows of n_q = K are the first K rows of n_q = K + 1, row 0 is the n_q=None result.  Anything
        else raises WavTokError or ValueError before any GPU work.
        normalize="peak" or "rms" (target_db, a peak target in dB, with "peak" alone): every clip is level-normalised first, the
        codes the bits of encode_codes(audio.normalize(audio_input, normalize, target_db)[0], ...); return_scales=True then returns
        (codes, scales (B,) fp32 on the device), the divisors, for decode_pcm(scales=...).  A target_db without "peak", an unknown
        mode and return_scales without normalize raise ValueError before any GPU work.
        normalize="lufs" (target_lufs, default -23): every clip is brought to that integrated loudness (ITU-R BS.1770-4 at the
        codec rate) as audio.normalize(audio_input, "lufs", target_lufs=...) does; a clip without a loudness (under 400 ms,
        silent) passes as it is with scale 1.  A target_lufs without "lufs" raises ValueError like the rest.
        max_true_peak_db (dBTP, with "lufs" only) bounds the gain by every clip's true peak, as audio.normalize(...,
        max_true_peak_db=...) does; given without "lufs", or no finite number: ValueError before any GPU work."""
        from . import audio as _audio
        self._check_bandwidth(bandwidth_id)
        norm = _audio.normalize_args("encode_codes", normalize, target_db, target_lufs)
        ceiling = _audio.ceiling_arg("encode_codes", normalize, max_true_peak_db)
        if norm is not None or return_scales:
            if norm is None:
                raise ValueError("encode_codes: return_scales needs normalize")
            if n_q is not None:
                n_q = self._check_n_q("encode_codes", n_q)
            assert audio_input.dim() == 2, "expected audio of shape (B, T)"
            dev = self._ensure_engine()
            rows = self._as_input(audio_input, dev).clone()
            scales = _audio.normalize_rows(rows, [rows.shape[1]] * rows.shape[0], *norm, sample_rate=self.codec_rate,
                                            max_true_peak_db=ceiling)
            codes = self.encode_codes(rows, n_q=n_q)
            return (codes, scales) if return_scales else codes
        if n_q is not None:
            n_q = self._check_n_q("encode_codes", n_q)
            assert audio_input.dim() == 2, "expected audio of shape (B, T)"
            dev = self._ensure_engine()
            audio = self._as_input(audio_input, dev)
            B, T = audio.shape
            return self._guarded(dev, lambda: self._encode_rvq(B, T, audio, n_q, self._graph_flags(B), dev), self._is_strict(B))[0]
        dev = self._ensure_engine()
        assert audio_input.dim() == 2, "expected audio of shape (B, T)"
        audio = self._as_input(audio_input, dev)
        B, T = audio.shape
        return self._guarded(dev, lambda: self._encode(B, T, audio, self._graph_flags(B), dev, want_emb=False, want_feats=False),
                             self._is_strict(B))[1]

    @property
    def codec_rate(self) -> int:
        return int(self.feature_extractor.encodec.sample_rate)

    def _bandwidth_index(self, bandwidth_id) -> int:
        if bandwidth_id is None:
            raise AssertionError("bandwidth_id is required (decoder/models.py:227)")
        if isinstance(bandwidth_id, torch.Tensor):
            if bandwidth_id.numel() != 1:
                raise ValueError("bandwidth_id must hold one index (the reference broadcasts a (1, dim) embedding row)")
            if bandwidth_id.device.type == "cpu":
                return int(bandwidth_id.reshape(-1)[0])
            # a tensor on the GPU: reading it is a device synchronisation, so the value is remembered per tensor object and
            # version for callers that build it once and pass it to every call.  Tensors made under torch.inference_mode()
            # carry no version counter (reading _version raises): those are read every time, like the reference's
            # infer.py:60-62 does with the new tensor it builds per file
            if bandwidth_id.is_inference():
                return int(bandwidth_id.reshape(-1)[0])
            c = self._bw_cache
            if c is not None and c[0]() is bandwidth_id and c[1] == bandwidth_id._version:
                return c[2]
            v = int(bandwidth_id.reshape(-1)[0])
            self._bw_cache = (weakref.ref(bandwidth_id), bandwidth_id._version, v)
            return v
        return int(bandwidth_id)

    def _check_bandwidth(self, bandwidth_id):
        """The encode side ignores bandwidth_id but for the reference's bounds check (feature_extractors.py:133): IndexError."""
        if bandwidth_id is not None:
            _ = self.feature_extractor.bandwidths[self._bandwidth_index(bandwidth_id)]

    def _run_decode(self, features: torch.Tensor, bandwidth_id, want_backbone: bool = False):
        dev = self._ensure_engine()
        assert features.dim() == 3 and features.shape[1] == self._arch.input_channels, "expected features (B, 512, L)"
        bw = self._bandwidth_index(bandwidth_id)
        features = self._as_input(features, dev)
        B = features.shape[0]
        # a call that wants the backbone output is never graph-replayed
        return self._guarded(dev, lambda: self._decode(features, bw, self._decode_flags(self._plan_flags if want_backbone else self._graph_flags(B)),
                                                       dev, want_backbone), self._is_strict(B))

    # -- decode straight from codes (WT_PLAN_DECODE_CODES / _MIXED): the plans gather the codebook rows themselves ------------
    def _codes_checked(self, dev: torch.device):
        """set_check_codes("sync") after a decode-from-codes call: wait for it and raise for a code outside the codebook."""
        if self._check_codes == "sync":
            torch.cuda.current_stream(dev).synchronize()
            self._poll_bad_codes()

    @torch.inference_mode()
    def decode_codes(self, codes: torch.Tensor, bandwidth_id=None) -> torch.Tensor:
        """decode(codes_to_features(codes), bandwidth_id=...) in one call, the same bits, without the (B, 512, L) feature
        tensor: codes (K, L) or (K, B, L) int64 as codes_to_features takes them -> (B, wave_len(L)).  The plan's first kernel
        gathers the codebook rows into the operand of backbone.embed.  A code outside the codebook follows set_check_codes
        like codes_to_features: "sync" raises IndexError for this call, "deferred" on the next call on this model, "off" never;
        the offending clip's waveform is NaN in every mode."""
        return self._run_decode_codes(codes, bandwidth_id)

    def _run_decode_codes(self, codes: torch.Tensor, bandwidth_id, borrow: bool = False) -> torch.Tensor:
        """decode_codes; with borrow a graph-replayed call returns the plan's staging buffer itself (_call)."""
        dev = self._ensure_engine()
        bw = self._bandwidth_index(bandwidth_id)
        if codes.dim() == 2:
            codes = codes.unsqueeze(1)
        assert codes.dim() == 3, "expected codes (K, L) or (K, B, L)"
        if not 1 <= codes.shape[0] <= self._arch.num_quantizers:      # (before a graph plan's staging buffer is filled)
            raise WavTokError("decode_codes: K must be between 1 and the number of codebooks", _capi.WT_ERR_INVALID)
        codes = self._as_input(codes, dev, torch.int64)
        B = codes.shape[1]
        wav = self._guarded(dev, lambda: self._decode_codes(codes, bw, self._decode_flags(self._graph_flags(B)), dev, borrow),
                            self._is_strict(B))[0]
        self._codes_checked(dev)
        return wav

    @torch.inference_mode()
    def decode_pcm(self, codes: torch.Tensor, sample_rate: Optional[int] = None, channels: int = 1, dtype: torch.dtype = torch.int16,
                   channels_last: bool = False, limit: float = 0.99, bandwidth_id=None, rescale: bool = False,
                   scales: Optional[torch.Tensor] = None) -> torch.Tensor:
        """decode_codes, then every clip resampled from the codec rate to sample_rate (default: the codec rate), expanded to
        `channels` (1, or 2: both channels carry the same samples, convert_audio's expand) and stored as fp32 or, clamped to
        [-limit, limit] and rounded like audio.to_pcm16, as int16: codes (K, L) or (K, B, L) -> (B, channels, n_out) or, with
        channels_last, (B, n_out, channels) on the model's device, n_out = ceil(sample_rate * wave_len(L) / 24000).  One
        decode_codes (graph-replayed where decode_codes is) and ONE ragged emit launch; with R = audio.convert_audio(
        decode_codes(codes)[:, None], 24000, sample_rate, 1) every channel of the fp32 result is the bits of R, of the int16 one
        the bits of audio.to_pcm16(R, limit=limit).  A code outside the codebook follows set_check_codes as in decode_codes; an
        int16 result no longer shows the NaN marker of a bad code (a NaN is clamped like any sample), so under "off" nothing
        reports it.  set_gemm_precision("f16") applies as to decode_codes.  Argument errors raise ValueError before any GPU
        work.
        rescale=True: save_audio's rescale (encoder/utils.py:95-103) per clip instead of the clamp, on the GPU (wt_emit_rescaled,
        two launches): clip b is the bits of audio.to_pcm16(R[b], rescale=True, limit=limit) (int16) or of R[b] times
        min(limit / max |R[b]|, 1) (fp32).  scales: (B,) from encode_codes(return_scales=True): row b of the decoded audio is
        multiplied by scales[b] in front of the emit (wt_scale_rows)."""
        from . import audio
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)):
            raise ValueError("decode_pcm: channels must be 1 or 2")
        (C,), fmt = self._emit_format("decode_pcm", channels, dtype, limit, 1)
        rate = self.codec_rate if sample_rate is None else int(sample_rate)
        audio.resampler_geometry(self.codec_rate, rate)                                     # (ValueError for a refused ratio)
        if not isinstance(codes, torch.Tensor) or codes.dim() not in (2, 3):
            raise ValueError("decode_pcm takes codes (K, L) or (K, B, L)")
        B, L = (1 if codes.dim() == 2 else int(codes.shape[1])), int(codes.shape[-1])
        n_in = self._wave_len(L)
        n_out = audio.resampled_length(self.codec_rate, rate, n_in)
        scales = self._check_scales("decode_pcm", scales, B)
        wav = self._run_decode_codes(codes, bandwidth_id, borrow=True)                      # (raises for a clip without samples)
        dev = wav.device
        if scales is not None:
            self._scale_rows(list(wav), [n_in] * B, scales, dev)
        out = torch.empty((B, n_out, C) if channels_last else (B, C, n_out), dtype=fmt[0], device=dev)
        spec = _PcmSpec(None, L, rate, n_in, n_out, C)
        self._emit_rows(list(wav), [spec] * B, out.view(-1), [b * n_out * C for b in range(B)], fmt, bool(channels_last), dev, bool(rescale))
        return out

    def _run_head(self, x: torch.Tensor) -> torch.Tensor:
        dev = self._ensure_engine()
        assert x.dim() == 3 and x.shape[2] == self._arch.dim, "expected the backbone output (B, L, dim)"
        x = self._as_input(x, dev)
        B, L, _ = x.shape
        outs = (((B, self._wave_len(L)), torch.float32, True),)
        return self._guarded(dev, lambda: self._call(lib.wt_head, _capi.WT_PLAN_HEAD, B, L, self._plan_flags, dev, (x,), outs),
                             self._is_strict(B))[0]

    def _run_seanet_decoder(self, z: torch.Tensor) -> torch.Tensor:
        dev = self._ensure_engine()
        z = self._as_input(z, dev)
        B, _, L = z.shape
        outs = (((B, 1, L * self._arch.hop), torch.float32, True),)
        return self._guarded(dev, lambda: self._call(lib.wt_seanet_decode, _capi.WT_PLAN_SEANET_DECODER, B, L, self._plan_flags,
                                                     dev, (z,), outs), self._is_strict(B))[0]

    def _run_unit_lstm(self, x: torch.Tensor) -> torch.Tensor:
        """Unit tests: the encoder's SLSTM alone, x (B, L, 512) time-major -> lstm(x) + x, on the plan's kernels."""
        dev = self._ensure_engine()
        x = self._as_input(x, dev)
        B, L, _ = x.shape
        (y,), _plan = self._call(lib.wt_unit_run, _capi.WT_PLAN_UNIT_LSTM, B, L, self._plan_flags, dev, (x,),
                                 ((x.shape, torch.float32, True),))
        return y

    def debug_stage(self, kind: int, B: int, length: int, name: str, rows: Optional[int] = None):
        """A named stage buffer of the cached plan (after a KEEP_STAGES run), decoded to fp32: returns (flat tensor,
        format bits); format & BUF_ELU says the buffer holds elu() of the reference's tensor.  S32 buffers are decoded
        (rows x cols with cols = numel / rows: pass `rows` for them)."""
        decode_kinds = (_capi.WT_PLAN_DECODE, _capi.WT_PLAN_DECODE_MIXED, _capi.WT_PLAN_DECODE_CODES, _capi.WT_PLAN_DECODE_CODES_MIXED)
        plan, ws = self._engine.plans[(kind, B, length, self._decode_flags(self._plan_flags) if kind in decode_kinds else self._plan_flags)]
        off, n, fmt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
        check(lib.wt_plan_buffer_info(plan, name.encode(), ctypes.byref(off), ctypes.byref(n), ctypes.byref(fmt)),
              "wt_plan_buffer_info")
        raw = ws[off.value: off.value + 4 * n.value]
        if fmt.value & _capi.BUF_S32:
            h = raw.view(torch.float16).view(-1, 2, 32).float()        # groups of [32 hi | 32 lo]
            return (h[:, 0, :] + h[:, 1, :] / 2048.0).reshape(-1), fmt.value
        return raw.view(torch.float32), fmt.value

    # -- reference API (pretrained.py:159-239) --------------------------------------------------------
    @torch.inference_mode()
    def forward(self, audio_input: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        features, _, _ = self.feature_extractor(audio_input, **kwargs)
        return self.decode(features, **kwargs)

    @torch.inference_mode()
    def encode(self, audio_input: torch.Tensor, **kwargs: Any):
        features, discrete_codes, _ = self.feature_extractor(audio_input, **kwargs)
        return features, discrete_codes

    @torch.inference_mode()
    def encode_infer(self, audio_input: torch.Tensor, **kwargs: Any):
        features, discrete_codes, _ = self.feature_extractor.infer(audio_input, **kwargs)
        return features, discrete_codes

    @torch.inference_mode()
    def decode(self, features_input: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        return self._run_decode(features_input, kwargs.get("bandwidth_id"))[0]

    @torch.inference_mode()
    def codes_to_features(self, codes: torch.Tensor) -> torch.Tensor:
        assert isinstance(self.feature_extractor, EncodecFeatures), \
            "Feature extractor should be an instance of EncodecFeatures"
        dev = self._ensure_engine()
        if codes.dim() == 2:
            codes = codes.unsqueeze(1)
        codes = self._as_input(codes, dev, torch.int64)
        K, B, L = codes.shape
        feats = torch.empty((B, 512, L), dtype=torch.float32, device=dev)
        check(lib.wt_codes_to_features(self._engine.model, _ptr(codes), K, B, L, _ptr(feats), _stream_ptr(dev)),
              "wt_codes_to_features")
        if self._check_codes == "sync":
            # F.embedding raises on an index outside the codebook (pretrained.py:236); the kernel flags it instead (and
            # writes NaN), which is read here after the (few microseconds of) work has completed
            torch.cuda.current_stream(dev).synchronize()
            self._poll_bad_codes()
        return feats
