"""The reference-shaped parameter tree: its callables hand their work to the ``WavTokenizer`` that owns them (``pretrained.py``)."""
from __future__ import annotations

import math
import weakref
from typing import Optional, Tuple

import torch
from torch import nn

from .config import ArchConfig
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
    """encodec.quantizer: the parameter holder, the reference's bandwidth arithmetic and encode (encoder/quantization/vq.py)."""

    def get_bandwidth_per_quantizer(self, frame_rate: int) -> float:      # vq.py:153-157
        """kbps one codebook adds: log2(bins) * frame_rate."""
        return math.log2(self.bins) * frame_rate

    def get_num_quantizers_for_bandwidth(self, frame_rate: int, bandwidth: Optional[float] = None) -> int:      # vq.py:142-151
        """Codebooks that fit `bandwidth` (kbps): all of them for None or a value <= 0, else
        max(1, floor(bandwidth * 1000 / (log2(bins) * frame_rate))); as in the reference the value is not cut to the number of
        layers here (encode does that: core_vq.py:407 takes layers[:n_q])."""
        n_q = self.n_q
        if bandwidth and bandwidth > 0.:
            n_q = int(max(1, math.floor(bandwidth * 1000 / self.get_bandwidth_per_quantizer(frame_rate))))
        return n_q

    @torch.inference_mode()
    def encode(self, x: torch.Tensor, frame_rate: int, bandwidth: Optional[float] = None) -> torch.Tensor:      # vq.py:159-168
        """Features (B, 512, L) -> codes (K, B, L) int64, K = get_num_quantizers_for_bandwidth(frame_rate, bandwidth) cut to the
        number of layers: greedy residual VQ (nearest row of codebook k to the residual, lowest index on ties; subtract in fp32;
        next codebook)."""
        return self._root()._run_quantize(x, min(self.get_num_quantizers_for_bandwidth(frame_rate, bandwidth), self.n_q))


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
        self._root()._check_bandwidth(bandwidth_id)
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
