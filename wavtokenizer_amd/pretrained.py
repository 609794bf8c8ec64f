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
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import yaml
from torch import nn

from . import _capi
from ._capi import WavTokError, WtArch, WtTensor, check, lib
from .config import ArchConfig, arch_from_yaml_dict
from .state_spec import full_state_spec, is_buffer


# ------------------------------------------------------------------ parameter containers
class _Holder(nn.Module):
    """Parameter/buffer container addressed by the reference's dotted state-dict keys."""

    def _put(self, dotted: str, tensor: torch.Tensor, buffer: bool):
        head, _, rest = dotted.partition(".")
        if rest:
            if head not in self._modules:
                self.add_module(head, _Holder())
            self._modules[head]._put(rest, tensor, buffer)
        elif buffer:
            self.register_buffer(head, tensor)
        else:
            self.register_parameter(head, nn.Parameter(tensor, requires_grad=False))

    def __getitem__(self, i):
        return self._modules[str(i)]

    def __len__(self):
        return len(self._modules)

    def __iter__(self):
        return iter(self._modules.values())

    def _bind(self, root):
        object.__setattr__(self, "_root", weakref.ref(root))
        for m in self._modules.values():
            if isinstance(m, _Holder):
                m._bind(root)


class SEANetEncoder(_Holder):
    """encodec.encoder: callable (B,1,T) -> (B,512,L) (encoder/modules/seanet.py:143)."""

    @torch.inference_mode()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        assert x.dim() == 3 and x.shape[1] == 1, "expected (B, 1, T)"
        return self._root()._run_encode(x[:, 0, :])[2]


class SEANetDecoder(_Holder):
    """encodec.decoder: callable (B,512,L) -> (B,1,L*hop) (encoder/modules/seanet.py:236-238)."""

    @torch.inference_mode()
    def forward(self, z: torch.Tensor) -> torch.Tensor:
        return self._root()._run_seanet_decoder(z)


class _CodebookLayer(_Holder):
    @property
    def codebook(self):                 # core_vq.py:274-276
        return self._modules["_codebook"].embed


class ResidualVectorQuantizer(_Holder):
    pass


class EncodecModel(_Holder):
    sample_rate = 24000
    channels = 1


class EncodecFeatures(_Holder):
    """decoder/feature_extractors.py:55-142 (container + infer)."""

    def forward(self, audio: torch.Tensor, bandwidth_id: torch.Tensor):
        # eval-mode quantiser forward picks n_q = 1 as well (vq.py:98-111), so it equals infer()
        return self.infer(audio, bandwidth_id)

    @torch.inference_mode()
    def infer(self, audio: torch.Tensor, bandwidth_id: torch.Tensor):
        _ = self.bandwidths[self._root()._bandwidth_index(bandwidth_id)] if bandwidth_id is not None else None
        feats, codes, _emb = self._root()._run_encode(audio, want_emb=False)
        # the third element of the reference's tuple (feature_extractors.py:141) is a zero scalar in eval mode; one cached
        # tensor per device instead of a fill kernel per call
        z = getattr(self, "_zero_loss", None)
        if z is None or z.device != audio.device:
            z = torch.zeros((), device=audio.device)
            object.__setattr__(self, "_zero_loss", z)
        return feats, codes, z


class VocosBackbone(_Holder):
    """decoder/models.py:223-235: callable (B,512,L) -> (B,L,dim)."""

    @torch.inference_mode()
    def forward(self, x: torch.Tensor, bandwidth_id: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert bandwidth_id is not None      # models.py:227
        return self._root()._run_decode(x, bandwidth_id, want_backbone=True)[1]


class ISTFTHead(_Holder):
    """decoder/heads.py:42-67: callable (B, L, dim) -> (B, L*hop)."""

    @torch.inference_mode()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._root()._run_head(x)


def _build_tree(arch: ArchConfig) -> Tuple[EncodecFeatures, VocosBackbone, ISTFTHead]:
    fe, bb, hd = EncodecFeatures(), VocosBackbone(), ISTFTHead()
    enc_model = EncodecModel()
    enc_model.add_module("encoder", SEANetEncoder())
    enc_model.add_module("quantizer", ResidualVectorQuantizer())
    enc_model.add_module("decoder", SEANetDecoder())
    fe.add_module("encodec", enc_model)
    q = enc_model.quantizer
    q.add_module("vq", _Holder())
    q.vq.add_module("layers", _Holder())
    for i in range(arch.num_quantizers):
        q.vq.layers.add_module(str(i), _CodebookLayer())
    q.bins = arch.vq_bins
    q.n_q = arch.num_quantizers
    q.dimension = 512
    fe.bandwidths = list(arch.bandwidths)
    fe.frame_rate = 25
    roots = {"feature_extractor": fe, "backbone": bb, "head": hd}
    for key, shape in full_state_spec(arch).items():
        top, _, rest = key.partition(".")
        t = torch.zeros(shape, dtype=torch.float32)
        roots[top]._put(rest, t, is_buffer(key))
    return fe, bb, hd


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


def _stream_ptr(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


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


def _decode_codes_mixed_entry(plan, codes, lengths, K, bw, wav, ws, stream):
    """lib.wt_decode_codes_mixed in the argument order of WavTokenizer._call (inputs, scalars, outputs)."""
    return lib.wt_decode_codes_mixed(plan, codes, K, lengths, bw, wav, ws, stream)


class _ClipSpec:
    """One clip of WavTokenizer.encode_codes_many: the tensor as given, its channels, samples per channel, layout, rate and
    resampled length."""
    __slots__ = ("clip", "channels", "n_in", "channels_last", "rate", "n_out")

    def __init__(self, clip: torch.Tensor, channels: int, n_in: int, channels_last: bool, rate: int, n_out: int):
        self.clip, self.channels, self.n_in, self.channels_last, self.rate, self.n_out = clip, channels, n_in, channels_last, rate, n_out


class _PcmSpec:
    """One clip of WavTokenizer.decode_pcm_many: its codes (K, L), frames, target rate, samples the decoder returns, samples per
    channel at the target rate and channels."""
    __slots__ = ("codes", "frames", "rate", "n_in", "n_out", "channels")

    def __init__(self, codes: Optional[torch.Tensor], frames: int, rate: int, n_in: int, n_out: int, channels: int):
        self.codes, self.frames, self.rate, self.n_in, self.n_out, self.channels = codes, frames, rate, n_in, n_out, channels


class _OffRoute(Exception):
    """A mixed-length call found the encoder off the route mixed-length plans take (WavTokenizer._mixed_route_ok)."""


# ------------------------------------------------------------------------------ public class
class WavTokenizer(nn.Module):
    """Same surface as the reference class (decoder/pretrained.py:32)."""

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
        if kind in (_capi.WT_PLAN_ENCODE, _capi.WT_PLAN_UNIT_LSTM):
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

        (feats, _codes, _emb), pe = self._encode(audio, flags, dev, want_emb=False)
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

    def _encode(self, audio: torch.Tensor, flags: int, dev: torch.device, want_emb: bool, want_feats: bool = True):
        """The encode call of _run_encode, encode_codes and range_report: ((features, codes, emb), plan).  Without want_feats a
        direct call passes a null features pointer (the library then skips the gather); a graph plan keeps passing its staging
        buffer, so encode_infer and encode_codes share one recording."""
        B, T = audio.shape
        L = self._arch.frames(T)
        return self._call(lib.wt_encode, _capi.WT_PLAN_ENCODE, B, T, flags, dev, (audio,),
                          (((B, 512, L), torch.float32, want_feats), ((1, B, L), torch.int64, True), ((B, 512, L), torch.float32, want_emb)),
                          name="wt_encode")

    def _run_encode(self, audio: torch.Tensor, want_emb: bool = True):
        dev = self._ensure_engine()
        assert audio.dim() == 2, "expected audio of shape (B, T)"
        audio = self._as_input(audio, dev)
        B = audio.shape[0]
        return self._guarded(dev, lambda: self._encode(audio, self._graph_flags(B), dev, want_emb), self._is_strict(B))

    def _run_encode_mixed(self, wavs: List[torch.Tensor], T_pad: int, dev: torch.device):
        """One mixed-length encode call (WT_PLAN_FLAG_MIXED_LENGTH) on clips of at least MIN_CLIP samples and at most T_pad:
        returns (features [B, 512, L_pad], codes [1, B, L_pad]) with -1 / 0 past each clip's frames, or None when the
        current flags or fp32 sites keep the encoder off the route a mixed-length plan takes (_mixed_route_ok; the caller
        then encodes the clips one at a time).  Any other refusal of the plan raises."""
        B = len(wavs)
        L = self._arch.frames(T_pad)
        lengths = [int(w.shape[0]) for w in wavs]

        def fill_wav(buf: torch.Tensor):        # (samples past a clip's length are never read)
            for j, w in enumerate(wavs):
                buf[j, :lengths[j]].copy_(w)

        ins = (((B, T_pad), torch.float32, fill_wav),
               ((B,), torch.int32, lambda lens: lens.copy_(torch.tensor(lengths, dtype=torch.int32), non_blocking=False)))
        outs = (((B, 512, L), torch.float32, True), ((1, B, L), torch.int64, True), None)      # (no emb output)

        def call():
            # checked on every attempt: a range fallback inside _guarded can put the encoder site on fp32
            if not self._mixed_route_ok():
                raise _OffRoute()
            return self._call(lib.wt_encode_mixed, _capi.WT_PLAN_ENCODE, B, T_pad,
                              self._graph_flags(B) | _capi.WT_PLAN_FLAG_MIXED_LENGTH, dev, ins, outs)

        try:
            return self._guarded(dev, call, self._is_strict(B))[:2]
        except _OffRoute:
            return None

    def _mixed_route_ok(self) -> bool:
        """Whether the encoder runs the route a mixed-length plan takes (the shipped split-f16 one): no fp32 GEMMs, no unfused
        debug plan, no debug taps or range report, the encoder range site not on fp32, and weights that fit the split-f16 form
        (the conditions build_encode checks; a plan refused in spite of them is an error, not a fallback)."""
        off_route = (_capi.WT_PLAN_FLAG_FP32_GEMM | _capi.WT_PLAN_FLAG_UNFUSED | _capi.WT_PLAN_FLAG_KEEP_STAGES |
                     _capi.WT_PLAN_FLAG_RANGE_REPORT)
        return (not (self._plan_flags & off_route) and not self._sites(_capi.WT_PLAN_ENCODE) and
                bool(lib.wt_model_split_ok(self._engine.model)))

    @torch.inference_mode()
    def encode_infer_many(self, wavs: Sequence[torch.Tensor], bandwidth_id=None) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """encode_infer over clips of different lengths (the reference's infer.py loop, one call per file) in a few batched
        calls: returns [(features [1, 512, L_i], codes [1, 1, L_i])] in input order, L_i = arch.frames(len(wavs[i])), each the
        same bits as encode_infer(wavs[i][None]).  Clips are sorted by length and grouped (mixed_length.group_clips: at most
        64 per call, padded to a coarse bucket so that calls share plans and graphs); clips shorter than the mixed-length
        plan's minimum, and every clip while the encoder runs off its shipped route (set_gemm_precision("f32"), an fp32
        encoder site after a range fallback, the unfused debug plans), run one at a time through encode_infer."""
        from .mixed_length import group_clips
        dev = self._ensure_engine()
        if bandwidth_id is not None:
            _ = self.feature_extractor.bandwidths[self._bandwidth_index(bandwidth_id)]
        wavs = list(wavs)
        for w in wavs:
            if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] < 1:
                raise ValueError("encode_infer_many takes a sequence of non-empty 1-D tensors")
        wavs = [self._as_input(w, dev) for w in wavs]
        out: List[Optional[Tuple[torch.Tensor, torch.Tensor]]] = [None] * len(wavs)
        groups, solo = group_clips([int(w.shape[0]) for w in wavs], self._arch.hop)
        for T_pad, idx in groups:
            res = self._run_encode_mixed([wavs[i] for i in idx], T_pad, dev)
            if res is None:
                solo.extend(idx)
                continue
            feats, codes = res
            for j, i in enumerate(idx):
                L_i = self._arch.frames(int(wavs[i].shape[0]))
                out[i] = (feats[j:j + 1, :, :L_i].clone(), codes[:, j:j + 1, :L_i].clone())
        for i in sorted(solo):
            out[i] = self.encode_infer(wavs[i][None], bandwidth_id=bandwidth_id)
        return out  # type: ignore[return-value]

    # -- tokenise straight from PCM: ragged ingest -> encode without a feature tensor -> ragged codes out ----------------------
    @torch.inference_mode()
    def encode_codes(self, audio_input: torch.Tensor, bandwidth_id=None) -> torch.Tensor:
        """encode_infer(audio_input, bandwidth_id=...)[1], the same bits, for a caller that wants the codes alone: (B, T) fp32 at
        the codec rate -> (1, B, L) int64.  A call that is not graph-replayed passes no feature buffer to the library (nothing
        gathers or writes the (B, 512, L) tensor); a graph-replayed one shares encode_infer's recording and staging buffers.
        Status, fallbacks and graphs behave as in encode_infer."""
        if bandwidth_id is not None:
            _ = self.feature_extractor.bandwidths[self._bandwidth_index(bandwidth_id)]
        dev = self._ensure_engine()
        assert audio_input.dim() == 2, "expected audio of shape (B, T)"
        audio = self._as_input(audio_input, dev)
        B = audio.shape[0]
        return self._guarded(dev, lambda: self._encode(audio, self._graph_flags(B), dev, want_emb=False, want_feats=False),
                             self._is_strict(B))[1]

    def _pinned(self, nbytes: int) -> Tuple[int, torch.Tensor]:
        """(slot, pinned uint8 buffer of at least nbytes): the two buffers take turns; a buffer whose last upload may still be
        running is waited for first."""
        k = self._pin_next
        self._pin_next ^= 1
        if self._pin_events[k] is not None:
            self._pin_events[k].synchronize()
        buf = self._pin_bufs[k]
        if buf is None or buf.numel() < nbytes:
            buf = self._pin_bufs[k] = torch.empty(max(nbytes + nbytes // 4, 1 << 20), dtype=torch.uint8, pin_memory=True)
        return k, buf

    def _ingest_stage(self, specs: Sequence["_ClipSpec"], offsets: Sequence[int], dev: torch.device):
        """Brings a group of clips within reach of one wt_ingest: the CPU clips, the resampled lengths (int32) and the code spans
        (int64 {frames, offset}) are packed into one pinned buffer and uploaded with ONE copy; clips on the GPU stay where they
        are.  Returns (descriptors, device workspace of wt_ingest, lengths on the GPU, spans on the GPU, what must stay alive)."""
        from . import audio
        B = len(specs)
        up = lambda n, a: -(-n // a) * a
        nbytes = lambda c: c.numel() * c.element_size()
        o_spans = up(4 * B, 8)
        pos = up(o_spans + 16 * B, 16)
        where = [-1] * B
        packed = []
        for j, sp in enumerate(specs):
            c = sp.clip
            if c.device.type != "cpu":
                if c.device != dev:
                    raise RuntimeError(f"a clip is on {c.device} but the model is on {dev}")
                continue
            packed.append(j)
            where[j] = pos
            pos = up(pos + nbytes(c), 16)
        slot, pin = self._pinned(pos)
        pin[:4 * B].view(torch.int32).copy_(torch.tensor([sp.n_out for sp in specs], dtype=torch.int32))
        spans = [v for sp, off in zip(specs, offsets) for v in (self._arch.frames(sp.n_out), int(off))]
        pin[o_spans:o_spans + 16 * B].view(torch.int64).copy_(torch.tensor(spans, dtype=torch.int64))
        for j in packed:
            c = specs[j].clip
            pin[where[j]:where[j] + nbytes(c)].view(c.dtype).view(c.shape).copy_(c)
        blob = torch.empty(pos, dtype=torch.uint8, device=dev)
        blob.copy_(pin[:pos], non_blocking=True)
        ev = self._pin_events[slot] = self._pin_events[slot] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        descs = (_capi.WtIngestClip * B)()
        blob_ptr = blob.data_ptr()
        handles: Dict[int, ctypes.c_void_p] = {}
        codec_rate = self.codec_rate
        for d, sp, o in zip(descs, specs, where):
            if o >= 0:           # packed contiguously in the clip's own shape
                st = (1,) if sp.clip.dim() == 1 else (int(sp.clip.shape[1]), 1)
                d.src = blob_ptr + o
            else:
                st = sp.clip.stride()
                d.src = sp.clip.data_ptr()
            d.dtype = _capi.WT_INGEST_I16 if sp.clip.dtype == torch.int16 else _capi.WT_INGEST_F32
            d.channels, d.n_in, d.n_out = sp.channels, sp.n_in, sp.n_out
            if sp.clip.dim() == 1:
                d.ch_stride, d.sample_stride = 0, st[0]
            else:
                d.ch_stride, d.sample_stride = (st[1], st[0]) if sp.channels_last else (st[0], st[1])
            if sp.rate not in handles:
                handles[sp.rate] = audio.resampler(sp.rate, codec_rate, dev.index)
            d.resampler = handles[sp.rate]
        ws = torch.empty(max(int(lib.wt_ingest_workspace_bytes(B)), 8), dtype=torch.uint8, device=dev)
        return descs, ws, blob[:4 * B].view(torch.int32), blob[o_spans:o_spans + 16 * B].view(torch.int64), (blob, [sp.clip for sp in specs])

    @property
    def codec_rate(self) -> int:
        return int(self.feature_extractor.encodec.sample_rate)

    def _run_encode_codes_mixed(self, specs: Sequence["_ClipSpec"], T_pad: int, flat: torch.Tensor, offsets: Sequence[int]):
        """One group of encode_codes_many: one upload, one wt_ingest into the plan's staging tensor, one wt_encode_mixed (no
        feature buffer unless the plan is graph-replayed), one wt_codes_unpack into flat at the clips' offsets.  Returns True, or
        None when the encoder is off the route a mixed-length plan takes (_mixed_route_ok)."""
        dev = self._ensure_engine()
        if not self._mixed_route_ok():          # (before anything is uploaded; checked again on every attempt below)
            return None
        B = len(specs)
        descs, ws, lengths, spans, _alive = self._ingest_stage(specs, offsets, dev)
        return self._encode_ingested_mixed(descs, ws, B, T_pad, lengths, spans, flat, dev)

    def _encode_ingested_mixed(self, descs, ws: torch.Tensor, B: int, T_pad: int, lengths: torch.Tensor, spans: torch.Tensor,
                               flat: torch.Tensor, dev: torch.device):
        """The launches of a mixed-length group whose wt_ingest descriptors, lengths (int32) and code spans (int64 {frames,
        offset}) are on hand, the latter two on the GPU: True, or None off the mixed route."""
        L = self._arch.frames(T_pad)

        def fill_wav(buf: torch.Tensor):        # (columns past a clip's length are never read)
            check(lib.wt_ingest(descs, B, T_pad, _ptr(buf), _ptr(ws), _stream_ptr(dev)), "wt_ingest")

        ins = (((B, T_pad), torch.float32, fill_wav), ((B,), torch.int32, lambda lens: lens.copy_(lengths)))
        # a graph plan passes its staging feature buffer like encode_infer_many (the recording is keyed by the pointers, so the two
        # alternate on one recording); a direct call passes none
        outs = (((B, 512, L), torch.float32, False), ((1, B, L), torch.int64, True), None)

        def call():
            if not self._mixed_route_ok():
                raise _OffRoute()
            return self._call(lib.wt_encode_mixed, _capi.WT_PLAN_ENCODE, B, T_pad,
                              self._graph_flags(B) | _capi.WT_PLAN_FLAG_MIXED_LENGTH, dev, ins, outs, name="wt_encode_mixed")

        try:
            codes = self._guarded(dev, call, self._is_strict(B))[1]
        except _OffRoute:
            return None
        check(lib.wt_codes_unpack(_ptr(codes), B, L, _ptr(spans), _ptr(flat), flat.numel(), _stream_ptr(dev)), "wt_codes_unpack")
        return True

    def _encode_codes_solo(self, specs: Sequence["_ClipSpec"], flat: torch.Tensor, offsets: Sequence[int]):
        """Clips that run one at a time (shorter than a mixed-length plan takes, or the encoder off its shipped route): ingested
        together like a group, at most MAX_GROUP per launch, then encode_codes per clip."""
        from .mixed_length import MAX_GROUP
        dev = self._ensure_engine()
        for c0 in range(0, len(specs), MAX_GROUP):
            part, offs = specs[c0:c0 + MAX_GROUP], offsets[c0:c0 + MAX_GROUP]
            T_pad = max(sp.n_out for sp in part)
            descs, ws, _lengths, _spans, _alive = self._ingest_stage(part, offs, dev)
            wav = torch.empty((len(part), T_pad), dtype=torch.float32, device=dev)
            check(lib.wt_ingest(descs, len(part), T_pad, _ptr(wav), _ptr(ws), _stream_ptr(dev)), "wt_ingest")
            for j, (sp, off) in enumerate(zip(part, offs)):
                codes = self.encode_codes(wav[j:j + 1, :sp.n_out])
                flat[off:off + codes.shape[-1]].copy_(codes.view(-1))

    def _clip_specs(self, who: str, clips: Sequence[torch.Tensor], sample_rates, channels_last: bool) -> List["_ClipSpec"]:
        """The clips of encode_codes_many / encode_codes_segmented_many, checked: ValueError for anything wt_ingest would refuse."""
        from . import audio
        clips = list(clips)
        codec_rate = self.codec_rate
        if sample_rates is None:
            rates = [codec_rate] * len(clips)
        elif isinstance(sample_rates, (int, np.integer)):
            rates = [int(sample_rates)] * len(clips)
        else:
            rates = [int(r) for r in sample_rates]
            if len(rates) != len(clips):
                raise ValueError(who + ": one sample rate, or one per clip")
        specs: List[_ClipSpec] = []
        for c, sr in zip(clips, rates):
            if not isinstance(c, torch.Tensor) or c.dim() not in (1, 2):
                raise ValueError(who + " takes tensors (T,), (C, T) or, with channels_last, (T, C)")
            if c.dtype not in (torch.float32, torch.int16):
                raise ValueError(who + " takes fp32 or int16 clips")
            ch = 1 if c.dim() == 1 else int(c.shape[1 if channels_last else 0])
            n_in = int(c.shape[0]) if c.dim() == 1 or channels_last else int(c.shape[1])
            if ch not in (1, 2):
                raise ValueError(who + ": audio must be mono or stereo")
            if n_in < 1:
                raise ValueError(who + ": empty clip")
            specs.append(_ClipSpec(c, ch, n_in, bool(channels_last and c.dim() == 2), sr,
                                   audio.resampled_length(sr, codec_rate, n_in)))       # (ValueError for a refused ratio)
        return specs

    @torch.inference_mode()
    def encode_codes_many(self, clips: Sequence[torch.Tensor], sample_rates=None, channels_last: bool = False, packed: bool = False,
                          bandwidth_id=None):
        """Tokenise a set of clips straight from PCM.  clips[i] is (T,), (C, T) or, with channels_last, (T, C), C in {1, 2}, fp32
        or int16 (scaled by 1 / 32768), on the CPU or on the model's device; sample_rates is one rate or one per clip (default:
        the codec rate).  Returns [codes (1, 1, L_i)] in input order, views into one flat int64 tensor, L_i =
        arch.frames(ceil(24000 * T_i / rate_i)); packed=True returns (that flat tensor [sum L_i], offsets [n + 1] on the CPU).
        Clip i's codes are the bits of encode_infer(audio.convert_audio(clip i as planar fp32, rate_i, 24000, 1)[0], ...)[1].
        Per group of encode_infer_many's grouping (on the resampled lengths): one upload of the group's CPU clips, one ragged
        ingest launch, one mixed-length encode without a feature tensor, one launch that hands out the codes.  Clips under the
        mixed-length plans' minimum, and every clip while the encoder is off its shipped route, are ingested the same way and
        encoded one at a time.  Argument errors raise ValueError before any GPU work."""
        from .mixed_length import group_clips
        if bandwidth_id is not None:
            _ = self.feature_extractor.bandwidths[self._bandwidth_index(bandwidth_id)]
        specs = self._clip_specs("encode_codes_many", clips, sample_rates, channels_last)
        offsets = [0]
        frames = self._arch.frames
        for sp in specs:
            offsets.append(offsets[-1] + frames(sp.n_out))
        flat = torch.empty(offsets[-1], dtype=torch.int64, device=self._device())
        groups, solo = group_clips([sp.n_out for sp in specs], self._arch.hop)
        for T_pad, idx in groups:
            if self._run_encode_codes_mixed([specs[i] for i in idx], T_pad, flat, [offsets[i] for i in idx]) is None:
                solo.extend(idx)
        if solo:
            solo = sorted(solo)
            self._encode_codes_solo([specs[i] for i in solo], flat, [offsets[i] for i in solo])
        if packed:
            return flat, torch.tensor(offsets, dtype=torch.int64)
        return [flat[offsets[i]:offsets[i + 1]].view(1, 1, -1) for i in range(len(specs))]

    # -- long recordings in overlapping segments (segmented.py): tokenise ---------------------------------------------------------
    def _upload_tables(self, tables: Sequence[torch.Tensor], dev: torch.device) -> List[torch.Tensor]:
        """Small host tensors (lengths, code spans, row pointers, weights) through one pinned buffer and ONE copy: their device twins."""
        up = lambda n: -(-n // 16) * 16
        where, pos = [], 0
        for t in tables:
            where.append(pos)
            pos = up(pos + t.numel() * t.element_size())
        if not pos:
            return [torch.empty(0, dtype=t.dtype, device=dev) for t in tables]
        slot, pin = self._pinned(pos)
        for t, o in zip(tables, where):
            pin[o:o + t.numel() * t.element_size()].view(t.dtype).copy_(t.reshape(-1))
        blob = torch.empty(pos, dtype=torch.uint8, device=dev)
        blob.copy_(pin[:pos], non_blocking=True)
        ev = self._pin_events[slot] = self._pin_events[slot] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        return [blob[o:o + t.numel() * t.element_size()].view(t.dtype).view(t.shape) for t, o in zip(tables, where)]

    def _encode_ingested_uniform(self, descs, ws: torch.Tensor, B: int, T: int, spans: torch.Tensor, flat: torch.Tensor, dev: torch.device):
        """One batch of B segments of one length T on the plain encode plan (encode_codes' own: same recording, same staging
        buffers), filled by one wt_ingest: True, or None when the encoder is off its shipped route (the segments then run one
        at a time, like a mixed-length group's)."""
        L = self._arch.frames(T)

        def fill_wav(buf: torch.Tensor):
            check(lib.wt_ingest(descs, B, T, _ptr(buf), _ptr(ws), _stream_ptr(dev)), "wt_ingest")

        ins = (((B, T), torch.float32, fill_wav),)
        outs = (((B, 512, L), torch.float32, False), ((1, B, L), torch.int64, True), ((B, 512, L), torch.float32, False))

        def call():
            if not self._mixed_route_ok():
                raise _OffRoute()
            return self._call(lib.wt_encode, _capi.WT_PLAN_ENCODE, B, T, self._graph_flags(B), dev, ins, outs, name="wt_encode")

        try:
            codes = self._guarded(dev, call, self._is_strict(B))[1]
        except _OffRoute:
            return None
        check(lib.wt_codes_unpack(_ptr(codes), B, L, _ptr(spans), _ptr(flat), flat.numel(), _stream_ptr(dev)), "wt_codes_unpack")
        return True

    @torch.inference_mode()
    def encode_codes_segmented_many(self, clips: Sequence[torch.Tensor], segment_length: int, stride: int, sample_rates=None,
                                    channels_last: bool = False, bandwidth_id=None):
        """Tokenise long recordings in overlapping segments (the reference's EncodecModel.encode, encoder/model.py:122-145).
        clips and sample_rates as encode_codes_many takes them (any rate, mono or stereo, planar or interleaved, fp32 or int16,
        on the CPU or on the model's device); segment_length and stride are samples at the codec rate, stride <= segment_length.
        Returns one segmented.SegmentedCodes per recording, all views of one flat int64 tensor.
        With W = audio.convert_audio(clip as planar fp32, rate, 24000, 1)[0] and (offsets, lengths) = segmented.segment_plan(
        len(W), segment_length, stride), segment i's codes are the bits of encode_codes(W[None, off_i:off_i + len_i]), whatever
        the other recordings, their order and the grouping: the recording is resampled first and cut second.  Near a cut the
        codes differ from the whole recording's by construction.
        Per <= 64 recordings one upload of the CPU clips and one ragged ingest launch write every W into one buffer; the segments
        are then wt_ingest descriptors at equal rates into W (no copy per segment): full segments fill uniform calls of up to 64
        on the plain encode plan, the short tails of all recordings share mixed-length groups (mixed_length.group_clips), each
        call one ingest launch, one encode without a feature tensor and one launch that hands out the codes.  Tails under the
        mixed-length plans' minimum, and every segment while the encoder is off its shipped route, are encoded one at a time.
        Status, fallbacks, strict mode and graphs behave as in encode_codes_many.  Argument errors (segmented.segment_plan's, a
        segment beyond 12 000 frames, an ISTFT head with padding="center") raise ValueError before any GPU work."""
        from . import audio
        from .mixed_length import MAX_GROUP, group_clips
        from .segmented import SegmentedCodes, check_geometry, segment_plan
        who = "encode_codes_segmented_many"
        if bandwidth_id is not None:
            _ = self.feature_extractor.bandwidths[self._bandwidth_index(bandwidth_id)]
        segment_plan(1, segment_length, stride)                 # (the geometry's own refusals, also for an empty list)
        specs = self._clip_specs(who, clips, sample_rates, channels_last)
        S, stride = int(segment_length), int(stride)
        seg_rec: List[int] = []                                  # per segment: recording, offset in W, samples, offset in flat
        seg_off: List[int] = []
        seg_len: List[int] = []
        seg_code: List[int] = []
        bounds = [0]                                             # per recording: its first segment's offset in flat
        rec_offsets: List[List[int]] = []
        for r, sp in enumerate(specs):
            offs, lens, frs = check_geometry(self._arch, sp.n_out, S, stride)
            pos = [bounds[-1]]
            for L in frs:
                pos.append(pos[-1] + L)
            seg_rec += [r] * len(offs)
            seg_off += offs
            seg_len += lens
            seg_code += pos[:-1]
            rec_offsets.append([v - pos[0] for v in pos])
            bounds.append(pos[-1])
        if not specs:
            return []
        dev = self._ensure_engine()
        flat = torch.empty(bounds[-1], dtype=torch.int64, device=dev)
        # every recording at the codec rate: W of recording r is row where[r][1] of the buffer where[r][0]
        where: List[Tuple[torch.Tensor, int]] = []
        c0 = 0
        while c0 < len(specs):
            c1, T_pad = c0, 0
            while c1 < len(specs) and c1 - c0 < MAX_GROUP and (c1 == c0 or (c1 - c0 + 1) * max(T_pad, specs[c1].n_out) <= 1 << 28):
                T_pad = max(T_pad, specs[c1].n_out)
                c1 += 1
            part = specs[c0:c1]
            descs, ws, _lengths, _spans, _alive = self._ingest_stage(part, [0] * len(part), dev)
            W = torch.empty((len(part), T_pad), dtype=torch.float32, device=dev)
            check(lib.wt_ingest(descs, len(part), T_pad, _ptr(W), _ptr(ws), _stream_ptr(dev)), "wt_ingest")
            where += [(W, j) for j in range(len(part))]
            c0 = c1
        frames = self._arch.frames
        on_route = self._mixed_route_ok()
        full = [k for k in range(len(seg_len)) if seg_len[k] == S] if on_route else []
        tails = [k for k in range(len(seg_len)) if seg_len[k] != S] if on_route else []
        groups, short = group_clips([seg_len[k] for k in tails], self._arch.hop)
        solo = [tails[i] for i in short] if on_route else list(range(len(seg_len)))
        # the calls: (padded length or 0 for a uniform batch, segments)
        calls = [(0, full[i:i + MAX_GROUP]) for i in range(0, len(full), MAX_GROUP)] + [(T_pad, [tails[i] for i in idx]) for T_pad, idx in groups]
        tables = []
        for _T, ks in calls:
            tables.append(torch.tensor([seg_len[k] for k in ks], dtype=torch.int32))
            tables.append(torch.tensor([v for k in ks for v in (frames(seg_len[k]), seg_code[k])], dtype=torch.int64))
        on_gpu = self._upload_tables(tables, dev)
        same = audio.resampler(self.codec_rate, self.codec_rate, dev.index)
        mixed_uniform = self._segment_uniform_mixed
        for n, (T_pad, ks) in enumerate(calls):
            B = len(ks)
            descs = (_capi.WtIngestClip * B)()
            for d, k in zip(descs, ks):
                W, j = where[seg_rec[k]]
                d.src = W.data_ptr() + 4 * (j * W.shape[1] + seg_off[k])
                d.dtype, d.channels, d.n_in, d.n_out = _capi.WT_INGEST_F32, 1, seg_len[k], seg_len[k]
                d.ch_stride, d.sample_stride, d.resampler = 0, 1, same
            ws = torch.empty(max(int(lib.wt_ingest_workspace_bytes(B)), 8), dtype=torch.uint8, device=dev)
            lengths, spans = on_gpu[2 * n], on_gpu[2 * n + 1]
            if T_pad == 0 and not mixed_uniform:
                done = self._encode_ingested_uniform(descs, ws, B, S, spans, flat, dev)
            else:
                done = self._encode_ingested_mixed(descs, ws, B, T_pad or S, lengths, spans, flat, dev)
            if not done:
                solo.extend(ks)
        for k in sorted(solo):
            W, j = where[seg_rec[k]]
            codes = self.encode_codes(W[j:j + 1, seg_off[k]:seg_off[k] + seg_len[k]])
            flat[seg_code[k]:seg_code[k] + codes.shape[-1]].copy_(codes.view(-1))
        return [SegmentedCodes(flat[bounds[r]:bounds[r + 1]], rec_offsets[r], sp.n_out, S, stride) for r, sp in enumerate(specs)]

    @torch.inference_mode()
    def encode_codes_segmented(self, clip: torch.Tensor, segment_length: int, stride: int, sample_rate: Optional[int] = None,
                               channels_last: bool = False, bandwidth_id=None):
        """encode_codes_segmented_many for one recording: its segmented.SegmentedCodes."""
        return self.encode_codes_segmented_many([clip], segment_length, stride, sample_rates=sample_rate, channels_last=channels_last,
                                                bandwidth_id=bandwidth_id)[0]

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

    def _run_decode(self, features: torch.Tensor, bandwidth_id, want_backbone: bool = False):
        dev = self._ensure_engine()
        assert features.dim() == 3 and features.shape[1] == self._arch.input_channels, "expected features (B, 512, L)"
        bw = self._bandwidth_index(bandwidth_id)
        features = self._as_input(features, dev)
        B = features.shape[0]
        # a call that wants the backbone output is never graph-replayed
        return self._guarded(dev, lambda: self._decode(features, bw, self._decode_flags(self._plan_flags if want_backbone else self._graph_flags(B)),
                                                       dev, want_backbone), self._is_strict(B))

    def _decode(self, features: torch.Tensor, bw: int, flags: int, dev: torch.device, want_backbone: bool):
        """The decode call of _run_decode and range_report: ((waveform, backbone output), plan)."""
        B, _, L = features.shape
        # no backbone buffer at all unless asked for: a graph plan's staging has none
        bb = ((B, L, self._arch.dim), torch.float32, True) if want_backbone else None
        return self._call(lib.wt_decode, _capi.WT_PLAN_DECODE, B, L, flags, dev, (features,),
                          (((B, self._wave_len(L)), torch.float32, True), bb), (bw,))

    def _run_decode_mixed(self, feats: List[torch.Tensor], L_pad: int, bw: int, dev: Optional[torch.device] = None):
        """One mixed-length decode call (WT_PLAN_DECODE_MIXED) on clips (512, L_i) of 1 <= L_i <= L_pad frames: returns the
        waveforms (B, wave_len(L_pad)), clip j's own samples first and zeros behind them, or None when the current flags or
        fp32 sites keep the decoder off the route a mixed-length plan takes (_decode_mixed_route_ok; the caller then decodes
        the clips one at a time).  Any other refusal of the plan raises."""
        dev = dev if dev is not None else self._ensure_engine()
        B = len(feats)
        lengths = [int(f.shape[1]) for f in feats]
        if min(lengths) < 1 or max(lengths) > L_pad:
            raise ValueError("every clip needs between 1 and L_pad frames")

        def fill_feats(buf: torch.Tensor):      # (frames past a clip's length are read and dropped by the first kernel)
            for j, f in enumerate(feats):
                buf[j, :, :lengths[j]].copy_(f)

        ins = (((B, self._arch.input_channels, L_pad), torch.float32, fill_feats),
               ((B,), torch.int32, lambda lens: lens.copy_(torch.tensor(lengths, dtype=torch.int32), non_blocking=False)))
        outs = (((B, self._wave_len(L_pad)), torch.float32, True),)

        def call():
            # checked on every attempt: a range fallback inside _guarded can put a decoder site on fp32
            if not self._decode_mixed_route_ok():
                raise _OffRoute()
            return self._call(lib.wt_decode_mixed, _capi.WT_PLAN_DECODE_MIXED, B, L_pad, self._decode_flags(self._graph_flags(B)), dev, ins, outs, (bw,))

        try:
            return self._guarded(dev, call, self._is_strict(B))[0]
        except _OffRoute:
            return None

    def _decode_mixed_route_ok(self) -> bool:
        """Whether the decoder runs the route a mixed-length plan takes (the shipped split-f16 one): no fp32 GEMMs, no unfused
        debug plan, no debug taps or range report, no decoder range site on fp32, and weights that fit the split-f16 form
        (the conditions build_decode checks; a plan refused in spite of them is an error, not a fallback).  The one-product mode
        (set_gemm_precision("f16")) is on the route: the mixed plans launch the same GEMMs."""
        off_route = (_capi.WT_PLAN_FLAG_FP32_GEMM | _capi.WT_PLAN_FLAG_UNFUSED | _capi.WT_PLAN_FLAG_KEEP_STAGES |
                     _capi.WT_PLAN_FLAG_RANGE_REPORT)
        return (not (self._plan_flags & off_route) and not self._sites(_capi.WT_PLAN_DECODE_MIXED) and
                bool(lib.wt_model_split_ok(self._engine.model)))

    @torch.inference_mode()
    def decode_many(self, features: Sequence[torch.Tensor], bandwidth_id=None) -> List[torch.Tensor]:
        """decode over clips of different lengths (the reference's infer.py loop, one call per file) in a few batched calls:
        features[i] is (512, L_i) or (1, 512, L_i) with L_i >= 1; returns [(1, wave_len(L_i))] in input order, each the same
        bits as decode(features[i][None], bandwidth_id=...), whatever the other clips and the grouping.  Clips are sorted by
        length and grouped (mixed_length.group_frames: at most 64 per call and at most MAX_SCORE_CELLS attention score cells,
        padded to a coarse bucket so that calls share plans and graphs).  A clip that forms a group alone, and every clip while
        the decoder runs off its shipped route (set_gemm_precision("f32"), an fp32 decoder site after a range fallback, the
        unfused debug plans), goes through decode."""
        from .mixed_length import group_frames
        dev = self._ensure_engine()
        bw = self._bandwidth_index(bandwidth_id)
        feats: List[torch.Tensor] = []
        for f in features:
            if isinstance(f, torch.Tensor) and f.dim() == 3 and f.shape[0] == 1:
                f = f[0]
            if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[0] != self._arch.input_channels or f.shape[1] < 1:
                raise ValueError("decode_many takes a sequence of tensors (512, L) or (1, 512, L) with L >= 1")
            feats.append(self._as_input(f, dev))
        out: List[Optional[torch.Tensor]] = [None] * len(feats)
        solo: List[int] = []
        min_frames = 1 if self._arch.padding == "same" else 2      # (decode raises for a 'center' clip of one frame)
        for L_pad, idx in group_frames([int(f.shape[1]) for f in feats]):
            if len(idx) == 1 or int(feats[idx[0]].shape[1]) < min_frames:
                solo.extend(idx)
                continue
            wav = self._run_decode_mixed([feats[i] for i in idx], L_pad, bw, dev)
            if wav is None:
                solo.extend(idx)
                continue
            for j, i in enumerate(idx):
                out[i] = wav[j:j + 1, :self._wave_len(int(feats[i].shape[1]))].clone()
        for i in sorted(solo):
            out[i] = self.decode(feats[i][None], bandwidth_id=bw)
        return out  # type: ignore[return-value]

    # -- decode straight from codes (WT_PLAN_DECODE_CODES / _MIXED): the plans gather the codebook rows themselves ------------
    def _codes_staging(self, K: int, B: int, L: int, flags: int, fill):
        """The codes input of a decode-from-codes _call.  K is an argument of the call, not of the plan, while a graph plan
        keeps ONE staging buffer: it is sized for every codebook, [num_quantizers][B][L], and a call fills its first K slabs
        (they are the call's [K][B][L] array; the recording is keyed by K).  fill(buf[:K]) writes them."""
        nq = self._arch.num_quantizers if flags & _capi.WT_PLAN_FLAG_GRAPH else K
        return ((nq, B, L), torch.int64, lambda buf: fill(buf[:K]))

    def _decode_codes(self, codes: torch.Tensor, bw: int, flags: int, dev: torch.device, borrow: bool = False):
        """The call of decode_codes: ((waveform, None), plan)."""
        K, B, L = codes.shape
        graph = flags & _capi.WT_PLAN_FLAG_GRAPH
        ins = (self._codes_staging(K, B, L, flags, lambda buf: buf.copy_(codes)),) if graph else (codes,)
        return self._call(lib.wt_decode_codes, _capi.WT_PLAN_DECODE_CODES, B, L, flags, dev, ins,
                          (((B, self._wave_len(L)), torch.float32, True), None), (K, bw), borrow=borrow)

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
    def _run_decode_codes_mixed(self, codes_list: List[torch.Tensor], L_pad: int, bw: int, dev: Optional[torch.device] = None,
                                borrow: bool = False):
        """One mixed-length decode-from-codes call (WT_PLAN_DECODE_CODES_MIXED) on clips (K, L_i) int64 of 1 <= L_i <= L_pad
        frames, the counterpart of _run_decode_mixed: returns the waveforms (B, wave_len(L_pad)), clip j's own samples first and
        zeros behind them, or None when the decoder is off the route a mixed-length plan takes (_decode_mixed_route_ok).  What
        the staging buffer holds past a clip's frames is never read.  borrow: as in _call."""
        dev = dev if dev is not None else self._ensure_engine()
        B = len(codes_list)
        K = int(codes_list[0].shape[0])
        lengths = [int(c.shape[1]) for c in codes_list]
        if min(lengths) < 1 or max(lengths) > L_pad:
            raise ValueError("every clip needs between 1 and L_pad frames")
        codes_list = [self._as_input(c, dev, torch.int64) for c in codes_list]

        def fill_codes(buf: torch.Tensor):
            for j, c in enumerate(codes_list):
                buf[:, j, :lengths[j]].copy_(c)

        outs = (((B, self._wave_len(L_pad)), torch.float32, True),)

        def call():
            # checked on every attempt: a range fallback inside _guarded can put a decoder site on fp32
            if not self._decode_mixed_route_ok():
                raise _OffRoute()
            flags = self._decode_flags(self._graph_flags(B))
            ins = (self._codes_staging(K, B, L_pad, flags, fill_codes),
                   ((B,), torch.int32, lambda lens: lens.copy_(torch.tensor(lengths, dtype=torch.int32), non_blocking=False)))
            return self._call(_decode_codes_mixed_entry, _capi.WT_PLAN_DECODE_CODES_MIXED, B, L_pad, flags, dev, ins, outs, (K, bw),
                              name="wt_decode_codes_mixed", borrow=borrow)

        try:
            wav = self._guarded(dev, call, self._is_strict(B))[0]
        except _OffRoute:
            return None
        self._codes_checked(dev)
        return wav

    def _codes_clips(self, codes: Sequence[torch.Tensor], who: str) -> List[torch.Tensor]:
        """The clips of decode_codes_many / decode_pcm_many as (K, L_i) tensors; ValueError for anything else."""
        clips: List[torch.Tensor] = []
        for c in codes:
            if isinstance(c, torch.Tensor) and c.dim() == 3 and c.shape[1] == 1:
                c = c[:, 0, :]
            if (not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] < 1 or c.is_floating_point() or c.is_complex()
                    or c.dtype == torch.bool):
                raise ValueError(who + " takes a sequence of integer tensors (K, L) or (K, 1, L) with L >= 1")
            if not 1 <= c.shape[0] <= self._arch.num_quantizers or c.shape[0] != (clips[0].shape[0] if clips else c.shape[0]):
                raise ValueError(who + ": every clip needs the same K, between 1 and the number of codebooks")
            clips.append(c)
        return clips

    @torch.inference_mode()
    def decode_codes_many(self, codes: Sequence[torch.Tensor], bandwidth_id=None) -> List[torch.Tensor]:
        """decode_codes over clips of different lengths in a few batched calls: codes[i] is (K, L_i) or (K, 1, L_i), an integer
        tensor, the same K throughout, L_i >= 1; returns [(1, wave_len(L_i))] in input order, each the same bits as
        decode_codes(codes[i], bandwidth_id=...) and as decode_many of its features.  The grouping is decode_many's
        (mixed_length.group_frames); a clip that forms a group alone, and every clip while the decoder runs off its shipped
        route, goes through decode_codes."""
        from .mixed_length import group_frames
        bw = self._bandwidth_index(bandwidth_id)
        clips = self._codes_clips(codes, "decode_codes_many")
        out: List[Optional[torch.Tensor]] = [None] * len(clips)
        solo: List[int] = []
        min_frames = 1 if self._arch.padding == "same" else 2      # (decode raises for a 'center' clip of one frame)
        for L_pad, idx in group_frames([int(c.shape[1]) for c in clips]):
            if len(idx) == 1 or int(clips[idx[0]].shape[1]) < min_frames:
                solo.extend(idx)
                continue
            wav = self._run_decode_codes_mixed([clips[i] for i in idx], L_pad, bw)
            if wav is None:
                solo.extend(idx)
                continue
            for j, i in enumerate(idx):
                out[i] = wav[j:j + 1, :self._wave_len(int(clips[i].shape[1]))].clone()
        for i in sorted(solo):
            out[i] = self.decode_codes(clips[i], bandwidth_id=bw)
        return out  # type: ignore[return-value]

    # -- synthesise straight to PCM: decode from codes -> ragged emit (resample, channels, layout, sample type) into one tensor -----
    def _emit_format(self, who: str, channels, dtype, limit, n: int) -> Tuple[List[int], Tuple[torch.dtype, float]]:
        """(channels per clip, (dtype, limit)) of decode_pcm / decode_pcm_many over n clips, checked: ValueError for anything
        wt_emit would refuse."""
        if dtype not in (torch.float32, torch.int16):
            raise ValueError(who + ": dtype must be torch.float32 or torch.int16")
        if isinstance(channels, (int, np.integer)):
            channels = [channels] * n
        channels = list(channels)
        if len(channels) != n:
            raise ValueError(who + ": one channel count, or one per clip")
        if any(isinstance(c, bool) or c not in (1, 2) for c in channels):
            raise ValueError(who + ": channels must be 1 or 2")
        limit = float(limit)
        if not 0.0 < limit <= 1.0:
            raise ValueError(who + ": limit must be in (0, 1]")
        return [int(c) for c in channels], (dtype, limit)

    def _emit_rows(self, rows: Sequence[torch.Tensor], specs: Sequence["_PcmSpec"], flat: torch.Tensor, offsets: Sequence[int],
                   fmt: Tuple[torch.dtype, float], channels_last: bool, dev: torch.device):
        """One wt_emit: rows[j], a contiguous fp32 row of at least specs[j].n_in samples at the codec rate on dev, goes to
        flat[offsets[j]:] at the clip's rate in the layout (channels, n_out) or, with channels_last, (n_out, channels)."""
        from . import audio
        dtype, limit = fmt
        B = len(rows)
        descs = (_capi.WtEmitClip * B)()
        base, esize = flat.data_ptr(), flat.element_size()
        codec_rate = self.codec_rate
        handles: Dict[int, ctypes.c_void_p] = {}
        for d, row, sp, off in zip(descs, rows, specs, offsets):
            channels = sp.channels
            assert row.dtype == torch.float32 and row.stride(-1) == 1 and row.shape[-1] >= sp.n_in and off + sp.n_out * channels <= flat.numel()
            if sp.rate not in handles:
                handles[sp.rate] = audio.resampler(codec_rate, sp.rate, dev.index)
            d.src, d.n_in, d.resampler, d.n_out = row.data_ptr(), sp.n_in, handles[sp.rate], sp.n_out
            d.dst = base + int(off) * esize
            d.dtype = _capi.WT_EMIT_I16 if dtype == torch.int16 else _capi.WT_EMIT_F32
            d.channels, d.limit = channels, limit
            if channels == 1:
                d.ch_stride, d.sample_stride = 0, 1
            else:
                d.ch_stride, d.sample_stride = (1, channels) if channels_last else (sp.n_out, 1)
        # up to 64 clips the library passes the descriptors with the launch and leaves the workspace alone: one small tensor serves
        # every such call; a larger launch gets a workspace of its own (the library fills it on the stream)
        if B <= 64:
            ws = self._emit_ws
            if ws is None or ws.device != dev:
                ws = self._emit_ws = torch.empty(max(int(lib.wt_emit_workspace_bytes(64)), 8), dtype=torch.uint8, device=dev)
        else:
            ws = torch.empty(int(lib.wt_emit_workspace_bytes(B)), dtype=torch.uint8, device=dev)
        check(lib.wt_emit(descs, B, _ptr(ws), _stream_ptr(dev)), "wt_emit")

    @torch.inference_mode()
    def decode_pcm(self, codes: torch.Tensor, sample_rate: Optional[int] = None, channels: int = 1, dtype: torch.dtype = torch.int16,
                   channels_last: bool = False, limit: float = 0.99, bandwidth_id=None) -> torch.Tensor:
        """decode_codes, then every clip resampled from the codec rate to sample_rate (default: the codec rate), expanded to
        `channels` (1, or 2: both channels carry the same samples, convert_audio's expand) and stored as fp32 or, clamped to
        [-limit, limit] and rounded like audio.to_pcm16, as int16: codes (K, L) or (K, B, L) -> (B, channels, n_out) or, with
        channels_last, (B, n_out, channels) on the model's device, n_out = ceil(sample_rate * wave_len(L) / 24000).  One
        decode_codes (graph-replayed where decode_codes is) and ONE ragged emit launch; with R = audio.convert_audio(
        decode_codes(codes)[:, None], 24000, sample_rate, 1) every channel of the fp32 result is the bits of R, of the int16 one
        the bits of audio.to_pcm16(R, limit=limit).  A code outside the codebook follows set_check_codes as in decode_codes; an
        int16 result no longer shows the NaN marker of a bad code (a NaN is clamped like any sample), so under "off" nothing
        reports it.  set_gemm_precision("f16") applies as to decode_codes.  Argument errors raise ValueError before any GPU
        work."""
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
        wav = self._run_decode_codes(codes, bandwidth_id, borrow=True)                      # (raises for a clip without samples)
        dev = wav.device
        out = torch.empty((B, n_out, C) if channels_last else (B, C, n_out), dtype=fmt[0], device=dev)
        spec = _PcmSpec(None, L, rate, n_in, n_out, C)
        self._emit_rows(list(wav), [spec] * B, out.view(-1), [b * n_out * C for b in range(B)], fmt, bool(channels_last), dev)
        return out

    def _run_decode_pcm_mixed(self, specs: Sequence["_PcmSpec"], L_pad: int, bw: int, flat: torch.Tensor, offsets: Sequence[int],
                              fmt: Tuple[torch.dtype, float], channels_last: bool):
        """One group of decode_pcm_many: one wt_decode_codes_mixed, one wt_emit from the plan's output rows into flat at the
        clips' offsets.  Returns True, or None when the decoder is off the route a mixed-length plan takes."""
        wav = self._run_decode_codes_mixed([sp.codes for sp in specs], L_pad, bw, borrow=True)
        if wav is None:
            return None
        self._emit_rows(list(wav), specs, flat, offsets, fmt, channels_last, wav.device)
        return True

    def _decode_pcm_solo(self, specs: Sequence["_PcmSpec"], bw: int, flat: torch.Tensor, offsets: Sequence[int],
                         fmt: Tuple[torch.dtype, float], channels_last: bool):
        """Clips that are decoded one at a time (a group of one, a 'center' clip under two frames, every clip while the decoder
        is off its mixed route): decode_codes per clip, then one wt_emit for the lot, at most MAX_GROUP clips per launch."""
        from .mixed_length import MAX_GROUP
        for c0 in range(0, len(specs), MAX_GROUP):
            part, offs = specs[c0:c0 + MAX_GROUP], offsets[c0:c0 + MAX_GROUP]
            rows = [self.decode_codes(sp.codes, bandwidth_id=bw)[0] for sp in part]
            self._emit_rows(rows, part, flat, offs, fmt, channels_last, rows[0].device)

    @torch.inference_mode()
    def decode_pcm_many(self, codes: Sequence[torch.Tensor], sample_rates=None, channels=1, dtype: torch.dtype = torch.int16,
                        channels_last: bool = False, limit: float = 0.99, packed: bool = False, device=None, bandwidth_id=None):
        """Synthesise a set of clips straight to PCM.  codes[i] is (K, L_i) or (K, 1, L_i) as decode_codes_many takes it;
        sample_rates is one rate or one per clip (default: the codec rate); channels is 1 or 2 for every clip, or one such
        count per clip; dtype, channels_last and limit as in decode_pcm.  Returns [pcm (channels, n_out_i)] or, with
        channels_last, [(n_out_i, channels)] in input order, n_out_i = ceil(rate_i * wave_len(L_i) / 24000), each a view into
        ONE flat tensor of sum n_out_i * channels_i elements;
        packed=True returns (that flat tensor, offsets [n + 1] on the CPU, in elements).  With R_i = audio.convert_audio(
        decode_codes(codes[i])[:, None], 24000, rate_i, 1), clip i is on every channel the bits of R_i (fp32) or of
        audio.to_pcm16(R_i, limit=limit) (int16), whatever the other clips, their order and the grouping.
        device="cpu" returns the flat tensor in pinned host memory: ONE device-to-host copy and one stream wait behind the last
        group; the default leaves everything on the model's device and waits for nothing.
        Per group of decode_codes_many's grouping: one mixed-length decode from codes and one ragged emit launch from the plan's
        output rows into the flat tensor (no copy per clip).  A clip that forms a group alone, a 'center' clip under two frames
        (decode_codes raises for it) and every clip while the decoder is off its mixed route are decoded one at a time and
        emitted together, at most 64 per launch.  A code outside the codebook follows set_check_codes as in decode_codes; an
        int16 result no longer shows the NaN marker of a bad code (a NaN is clamped like any sample), so under "off" nothing
        reports it.  Argument errors raise ValueError before any GPU work."""
        from . import audio
        from .mixed_length import group_frames
        who = "decode_pcm_many"
        bw = self._bandwidth_index(bandwidth_id)
        clips = self._codes_clips(codes, who)
        chans, fmt = self._emit_format(who, channels, dtype, limit, len(clips))
        channels_last = bool(channels_last)
        codec_rate = self.codec_rate
        rates, to_host = self._pcm_rates_device(who, len(clips), sample_rates, device)
        specs: List[_PcmSpec] = []
        offsets = [0]
        for c, sr, ch in zip(clips, rates, chans):
            L = int(c.shape[1])
            n_in = self._wave_len(L)
            n_out = audio.resampled_length(codec_rate, sr, n_in)                            # (ValueError for a refused ratio)
            specs.append(_PcmSpec(c, L, sr, n_in, n_out, ch))
            offsets.append(offsets[-1] + n_out * ch)
        flat = torch.empty(offsets[-1], dtype=fmt[0], device=self._device())
        solo: List[int] = []
        min_frames = 1 if self._arch.padding == "same" else 2      # (decode_codes raises for a 'center' clip of one frame)
        for L_pad, idx in group_frames([sp.frames for sp in specs]):
            if len(idx) == 1 or specs[idx[0]].frames < min_frames:
                solo.extend(idx)
                continue
            if self._run_decode_pcm_mixed([specs[i] for i in idx], L_pad, bw, flat, [offsets[i] for i in idx], fmt, channels_last) is None:
                solo.extend(idx)
        if solo:
            solo = sorted(solo)
            self._decode_pcm_solo([specs[i] for i in solo], bw, flat, [offsets[i] for i in solo], fmt, channels_last)
        return self._pcm_result(flat, offsets, specs, packed, to_host, channels_last)

    def _pcm_rates_device(self, who: str, n: int, sample_rates, device) -> Tuple[List[int], bool]:
        """(rate per clip, whether the result goes to the host) of decode_pcm_many / decode_pcm_segmented_many, checked."""
        if sample_rates is None:
            rates = [self.codec_rate] * n
        elif isinstance(sample_rates, (int, np.integer)):
            rates = [int(sample_rates)] * n
        else:
            rates = [int(r) for r in sample_rates]
            if len(rates) != n:
                raise ValueError(who + ": one sample rate, or one per clip")
        to_host = device is not None and torch.device(device).type == "cpu"
        if device is not None and not to_host:
            want, own = torch.device(device), self._device()
            if want.type != own.type or (want.index is not None and want.index != (own.index if own.index is not None else 0)):
                raise ValueError(who + ": device is None, the model's own device or 'cpu'")
        return rates, to_host

    @staticmethod
    def _pcm_result(flat: torch.Tensor, offsets: Sequence[int], specs: Sequence["_PcmSpec"], packed: bool, to_host: bool, channels_last: bool):
        """What decode_pcm_many and decode_pcm_segmented_many return: the flat tensor (to_host: through ONE copy into pinned memory
        and one stream wait) with its offsets, or the clips' views of it."""
        if to_host:
            host = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
            if flat.numel():
                host.copy_(flat, non_blocking=True)
                torch.cuda.current_stream(flat.device).synchronize()
            flat = host
        if packed:
            return flat, torch.tensor(offsets, dtype=torch.int64)
        return [flat[offsets[i]:offsets[i + 1]].view((sp.n_out, sp.channels) if channels_last else (sp.channels, sp.n_out))
                for i, sp in enumerate(specs)]

    # -- long recordings in overlapping segments (segmented.py): synthesise -------------------------------------------------------
    @torch.inference_mode()
    def decode_pcm_segmented_many(self, segs, sample_rates=None, channels=1, dtype: torch.dtype = torch.int16, channels_last: bool = False,
                                  limit: float = 0.99, packed: bool = False, device=None, bandwidth_id=None):
        """Synthesise long recordings from their segments' codes (the reference's EncodecModel.decode, encoder/model.py:167-178):
        segs[r] is a segmented.SegmentedCodes, from encode_codes_segmented(_many) or built by hand; the other arguments and the
        forms of the result (views of one flat tensor, packed=True, device="cpu" into pinned memory with one copy and one wait)
        are decode_pcm_many's, with n_out_r = ceil(rate_r * length_r / 24000).
        With X = audio.linear_overlap_add([decode_codes(c_i)[..., :len_i] for i], stride)[..., :length] over recording r's
        segments, every channel of the result is the bits of audio.convert_audio(X[:, None], 24000, rate_r, 1) (fp32) or of
        audio.to_pcm16(that, limit=limit) (int16), whatever the other recordings and the grouping.
        All segments of all recordings are decoded in groups: segments of a full segment's frame count in decode_codes batches of
        up to 64 (fewer where the attention score cells say so), the tails through decode_codes_many's grouping; then, per <= 64
        recordings, one ragged overlap-add launch (wt_overlap_add_ragged) reads the decoded rows where those calls left them,
        through a device table of row pointers, into one 24 kHz row per recording, and one wt_emit converts those rows.  The
        decoded segments stay allocated until the overlap-add is enqueued: about length * segment_length / stride floats per
        recording, plus one 24 kHz row each.  set_gemm_precision("f16"), set_check_codes and the fallbacks apply as to
        decode_codes (under "sync" there is one wait behind the last uniform batch, not one per batch).  Argument errors
        (SegmentedCodes.validate's among them: offsets or length that contradict segment_plan, padding="center") raise
        ValueError before any GPU work."""
        from . import audio
        from .mixed_length import MAX_GROUP, MAX_SCORE_CELLS, group_frames, score_cells
        from .segmented import SegmentedCodes
        who = "decode_pcm_segmented_many"
        bw = self._bandwidth_index(bandwidth_id)
        segs = list(segs)
        if any(not isinstance(sc, SegmentedCodes) for sc in segs):
            raise ValueError(who + " takes a sequence of segmented.SegmentedCodes")
        geo = [sc.validate(self._arch) for sc in segs]
        chans, fmt = self._emit_format(who, channels, dtype, limit, len(segs))
        channels_last = bool(channels_last)
        rates, to_host = self._pcm_rates_device(who, len(segs), sample_rates, device)
        specs: List[_PcmSpec] = []
        offsets = [0]
        for sc, sr, ch in zip(segs, rates, chans):
            n_out = audio.resampled_length(self.codec_rate, sr, sc.length)                  # (ValueError for a refused ratio)
            specs.append(_PcmSpec(None, int(sc.offsets[-1]), sr, sc.length, n_out, ch))
            offsets.append(offsets[-1] + n_out * ch)
        if not segs:
            return self._pcm_result(torch.empty(0, dtype=fmt[0], device=self._device()), offsets, specs, packed, to_host, channels_last)
        dev = self._ensure_engine()
        flat = torch.empty(offsets[-1], dtype=fmt[0], device=dev)
        codes = [sc.codes.to(device=dev, dtype=torch.int64).contiguous() for sc in segs]
        # every segment of every recording: (recording, segment, first code, frames)
        items = [(r, i, int(o), L) for r, sc in enumerate(segs) for i, (o, L) in enumerate(zip(sc.offsets.tolist(), geo[r][2]))]
        on_route = self._decode_mixed_route_ok()
        full_frames = {geo[r][2][0] for r, sc in enumerate(segs) if geo[r][1][0] == sc.segment_length} if on_route else set()
        rows: List[List[Optional[torch.Tensor]]] = [[None] * sc.n_segments for sc in segs]      # (they keep the decoded batches alive)
        solo: List[int] = [] if on_route else list(range(len(items)))
        by_frames: Dict[int, List[int]] = {}
        rest: List[int] = []
        for k, (_r, _i, _o, L) in enumerate(items):
            if L in full_frames:
                by_frames.setdefault(L, []).append(k)
            elif on_route:
                rest.append(k)
        for L, ks in by_frames.items():
            per_call = max(1, min(MAX_GROUP, MAX_SCORE_CELLS // score_cells(1, L)))
            for c0 in range(0, len(ks), per_call):
                part = ks[c0:c0 + per_call]
                B = len(part)
                runs: List[List[int]] = []                           # consecutive segments of one recording are one slice of its codes
                for k in part:
                    r, _i, o, _L = items[k]
                    if runs and runs[-1][0] == r and runs[-1][2] == o:
                        runs[-1][2] = o + L
                    else:
                        runs.append([r, o, o + L])
                pieces = [codes[r][a:b] for r, a, b in runs]
                batch = (pieces[0] if len(pieces) == 1 else torch.cat(pieces)).view(1, B, L)

                def call():
                    if not self._decode_mixed_route_ok():
                        raise _OffRoute()
                    return self._decode_codes(batch, bw, self._decode_flags(self._graph_flags(B)), dev)

                try:
                    wav = self._guarded(dev, call, self._is_strict(B))[0]
                except _OffRoute:
                    solo.extend(part)
                    continue
                for j, k in enumerate(part):
                    rows[items[k][0]][items[k][1]] = wav[j]
        if by_frames:
            self._codes_checked(dev)
        seg_codes = lambda k: codes[items[k][0]][items[k][2]:items[k][2] + items[k][3]].view(1, -1)
        for L_pad, idx in group_frames([items[k][3] for k in rest]):
            part = [rest[i] for i in idx]
            wav = self._run_decode_codes_mixed([seg_codes(k) for k in part], L_pad, bw, dev) if len(part) > 1 else None
            if wav is None:
                solo.extend(part)
                continue
            for j, k in enumerate(part):
                rows[items[k][0]][items[k][1]] = wav[j]
        for k in sorted(solo):
            rows[items[k][0]][items[k][1]] = self.decode_codes(seg_codes(k), bandwidth_id=bw)[0]
        # the cross-fade: one launch per <= 64 recordings from one upload of the row pointers and the triangles
        x_off = [0]
        for sc in segs:
            x_off.append(x_off[-1] + -(-sc.length // 4) * 4)         # (rows start on 16 bytes: wt_emit's wide loads)
        X = torch.empty(x_off[-1], dtype=torch.float32, device=dev)
        flens = sorted({min(sc.segment_length, sc.length) for sc in segs})
        tri = []
        for flen in flens:                                           # the reference's triangle, from the same torch.linspace
            t = torch.linspace(0, 1, flen + 2, dtype=torch.float32)[1:-1]
            tri.append(0.5 - (t - 0.5).abs())
        ptrs = torch.tensor([row.data_ptr() for rr in rows for row in rr], dtype=torch.int64)
        on_gpu = self._upload_tables([ptrs] + tri, dev)
        table, weight = on_gpu[0], dict(zip(flens, on_gpu[1:]))
        first = [0]
        for sc in segs:
            first.append(first[-1] + sc.n_segments)
        for c0 in range(0, len(segs), MAX_GROUP):
            part = range(c0, min(c0 + MAX_GROUP, len(segs)))
            descs = (_capi.WtOverlapAddClip * len(part))()
            for d, r in zip(descs, part):
                sc = segs[r]
                flen = min(sc.segment_length, sc.length)
                assert all(row.shape[-1] >= n for row, n in zip(rows[r], geo[r][1]))
                d.rows = table.data_ptr() + 8 * first[r]
                d.n_frames, d.frame_len, d.stride, d.total = sc.n_segments, flen, sc.stride, sc.length
                d.weight, d.out = weight[flen].data_ptr(), X.data_ptr() + 4 * x_off[r]
            ws = torch.empty(max(int(lib.wt_overlap_add_ragged_workspace_bytes(len(part))), 8), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                check(lib.wt_overlap_add_ragged(descs, len(part), _ptr(ws), _stream_ptr(dev)), "wt_overlap_add_ragged")
            self._emit_rows([X[x_off[r]:x_off[r] + segs[r].length] for r in part], [specs[r] for r in part], flat,
                            [offsets[r] for r in part], fmt, channels_last, dev)
        return self._pcm_result(flat, offsets, specs, packed, to_host, channels_last)

    @torch.inference_mode()
    def decode_pcm_segmented(self, seg, sample_rate: Optional[int] = None, channels: int = 1, dtype: torch.dtype = torch.int16,
                             channels_last: bool = False, limit: float = 0.99, packed: bool = False, device=None, bandwidth_id=None):
        """decode_pcm_segmented_many for one recording: (channels, n_out) or, with channels_last, (n_out, channels); packed=True
        returns the flat tensor and its offsets."""
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)):
            raise ValueError("decode_pcm_segmented: channels must be 1 or 2")
        out = self.decode_pcm_segmented_many([seg], sample_rates=sample_rate, channels=channels, dtype=dtype, channels_last=channels_last,
                                             limit=limit, packed=packed, device=device, bandwidth_id=bandwidth_id)
        return out if packed else out[0]

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
