"""The calls of ``WavTokenizer`` that take many clips at once, and the parts they share: the route check and the guarded
mixed-length call, the grouped driver, the pinned upload, the wt_ingest and wt_emit descriptors."""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from ._capi import check, lib
from .engine import _ptr, _stream_ptr


# one clip of encode_codes_many: the tensor as given, its channels, samples per channel, layout, rate and resampled length
_ClipSpec = namedtuple("_ClipSpec", "clip channels n_in channels_last rate n_out")
# one clip of decode_pcm_many: codes (K, L) or None, frames, target rate, samples decoded, samples per channel at that rate, channels
_PcmSpec = namedtuple("_PcmSpec", "codes frames rate n_in n_out channels")


class _OffRoute(Exception):
    """A mixed-length call found the model off the route mixed-length plans take (_BatchedCalls._route_ok)."""


class _BatchedCalls:
    """The batched calls of WavTokenizer, methods alone: state, _call, _guarded and the staging layouts are WavTokenizer's own."""

    def _route_ok(self, kind: int) -> bool:
        """Whether the side of the model that plan kind belongs to runs the route a mixed-length plan takes (the shipped split-f16
        one): no fp32 GEMMs, no unfused debug plan, no debug taps or range report, none of the kind's range sites on fp32, and
        weights that fit the split-f16 form (the conditions build_encode / build_decode check; a plan refused in spite of them
        is an error, not a fallback).  set_gemm_precision("f16") is on the route: the mixed plans launch the same GEMMs.
        The encoder side also needs the architecture's first stage on the kernel that holds its down conv (resblock16.hip: a
        first encoder ratio of 2 or 4): it is the one stage-1 form that takes per-clip lengths, so a model with another first
        ratio (a build_encode condition like the rest) encodes its clips one at a time."""
        off_route = (_capi.WT_PLAN_FLAG_FP32_GEMM | _capi.WT_PLAN_FLAG_UNFUSED | _capi.WT_PLAN_FLAG_KEEP_STAGES |
                     _capi.WT_PLAN_FLAG_RANGE_REPORT)
        if kind == _capi.WT_PLAN_ENCODE and self._arch.enc_ratios[0] not in (2, 4):
            return False
        return not (self._plan_flags & off_route) and not self._sites(kind) and bool(lib.wt_model_split_ok(self._engine.model))

    def _guarded_mixed(self, kind: int, B: int, thunk, dev: torch.device):
        """The outputs of thunk() -> (outputs, plan), one _call on a plan that exists on the mixed route alone, under _guarded;
        None when the model is off that route (the caller then takes the clips one at a time; any other refusal raises).  The
        route is checked on every attempt: a range fallback inside _guarded can put one of the kind's sites on fp32."""
        def call():
            if not self._route_ok(kind):
                raise _OffRoute()
            return thunk()

        try:
            return self._guarded(dev, call, self._is_strict(B))
        except _OffRoute:
            return None

    @staticmethod
    def _run_groups(groups, solo: Sequence[int], run_group, run_solo):
        """The driver of every batched call: run_group(pad, idx) per group; the clips of a group it answers with None (the model
        is off the mixed route) join `solo`, the clips no group takes, and run_solo gets them all, sorted, in one call."""
        solo = list(solo)
        for pad, idx in groups:
            if run_group(pad, idx) is None:
                solo.extend(idx)
        if solo:
            run_solo(sorted(solo))

    def _run_groups_of(self, specs, offsets, groups, solo, run_group, run_solo):
        """_run_groups for the calls that write every clip's result into one flat tensor at its offset: run_group(pad, specs of
        the group, their offsets), run_solo(specs of the remainder, their offsets)."""
        pick = lambda idx: ([specs[i] for i in idx], [offsets[i] for i in idx])
        self._run_groups(groups, solo, lambda pad, idx: run_group(pad, *pick(idx)), lambda idx: run_solo(*pick(idx)))

    def _decode_groups(self, frames: Sequence[int]):
        """mixed_length.group_frames as (groups, solo), the form of group_clips: a clip that forms a group alone and a 'center'
        clip under two frames (decode raises for it) are decoded one at a time."""
        from .mixed_length import group_frames
        min_frames = 1 if self._arch.padding == "same" else 2
        groups, solo = [], []
        for L_pad, idx in group_frames(frames):
            if len(idx) == 1 or frames[idx[0]] < min_frames:
                solo.extend(idx)
            else:
                groups.append((L_pad, idx))
        return groups, solo

    @staticmethod
    def _per_clip(value, n: int, error: str, convert=lambda v: v) -> list:
        """An argument that is one value for every clip or one per clip, as a list of n converted values."""
        if isinstance(value, (int, np.integer)):
            return [convert(value)] * n
        value = [convert(v) for v in value]
        if len(value) != n:
            raise ValueError(error)
        return value

    def _rates(self, who: str, sample_rates, n: int) -> List[int]:
        rates = self.codec_rate if sample_rates is None else sample_rates
        return self._per_clip(rates, n, who + ": one sample rate, or one per clip", int)

    def _run_encode_mixed(self, wavs: List[torch.Tensor], T_pad: int, dev: torch.device):
        """One mixed-length encode call (WT_PLAN_FLAG_MIXED_LENGTH) on clips of at least MIN_CLIP samples and at most T_pad:
        returns (features [B, 512, L_pad], codes [1, B, L_pad]) with -1 / 0 past each clip's frames, or None when the
        current flags or fp32 sites keep the encoder off the route a mixed-length plan takes (_route_ok; the caller
        then encodes the clips one at a time).  Any other refusal of the plan raises."""
        B = len(wavs)
        lengths = [int(w.shape[0]) for w in wavs]

        def fill_wav(buf: torch.Tensor):
            for j, w in enumerate(wavs):
                buf[j, :lengths[j]].copy_(w)

        res = self._guarded_mixed(_capi.WT_PLAN_ENCODE, B, lambda: self._encode_mixed(B, T_pad, fill_wav, lengths, dev, True), dev)
        return res and res[:2]

    @torch.inference_mode()
    def encode_infer_many(self, wavs: Sequence[torch.Tensor], bandwidth_id=None) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """encode_infer over clips of different lengths (the reference's infer.py loop, one call per file) in a few batched
        calls: returns [(features [1, 512, L_i], codes [1, 1, L_i])] in input order, L_i = arch.frames(len(wavs[i])), each the
        same bits as encode_infer(wavs[i][None]).  Clips are sorted by length and grouped (mixed_length.group_clips: at most
        64 per call, padded to a coarse bucket so that calls share plans and graphs); clips shorter than the mixed-length
        plan's minimum, and every clip while the encoder runs off its shipped route (set_gemm_precision("f32"), an fp32
        encoder site after a range fallback, the unfused debug plans), run one at a time through encode_infer.  So does every
        clip of a model whose first encoder ratio (the last of arch.ratios) is neither 2 nor 4: the mixed-length plan needs the
        stage-1 kernel that holds the down conv (_route_ok)."""
        from .mixed_length import group_clips
        dev = self._ensure_engine()
        self._check_bandwidth(bandwidth_id)
        wavs = list(wavs)
        for w in wavs:
            if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] < 1:
                raise ValueError("encode_infer_many takes a sequence of non-empty 1-D tensors")
        wavs = [self._as_input(w, dev) for w in wavs]
        out: List[Optional[Tuple[torch.Tensor, torch.Tensor]]] = [None] * len(wavs)

        def run_group(T_pad, idx):
            res = self._run_encode_mixed([wavs[i] for i in idx], T_pad, dev)
            if res is None:
                return None
            feats, codes = res
            for j, i in enumerate(idx):
                L_i = self._arch.frames(int(wavs[i].shape[0]))
                out[i] = (feats[j:j + 1, :, :L_i].clone(), codes[:, j:j + 1, :L_i].clone())
            return True

        def run_solo(idx):
            for i in idx:
                out[i] = self.encode_infer(wavs[i][None], bandwidth_id=bandwidth_id)

        self._run_groups(*group_clips([int(w.shape[0]) for w in wavs], self._arch.hop), run_group, run_solo)
        return out  # type: ignore[return-value]

    # -- tokenise straight from PCM: ragged ingest -> encode without a feature tensor -> ragged codes out ----------------------
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

    def _upload(self, tables: Sequence[torch.Tensor], dev: torch.device) -> Tuple[torch.Tensor, List[int]]:
        """Host tensors (lengths, code spans, row pointers, weights, a group's CPU clips) through one pinned buffer and ONE copy:
        (the blob on the GPU, each table's byte offset in it); a table lies there contiguous, in its own shape, on 16 bytes."""
        where, ends, pos = [], [], 0
        for t in tables:
            where.append(pos)
            ends.append(pos + t.numel() * t.element_size())
            pos = -(-ends[-1] // 16) * 16
        blob = torch.empty(pos, dtype=torch.uint8, device=dev)
        if pos:
            slot, pin = self._pinned(pos)
            for t, o, end in zip(tables, where, ends):
                pin[o:end].view(t.dtype).view(t.shape).copy_(t)
            blob.copy_(pin[:pos], non_blocking=True)
            ev = self._pin_events[slot] = self._pin_events[slot] or torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
        return blob, where

    def _upload_tables(self, tables: Sequence[torch.Tensor], dev: torch.device) -> List[torch.Tensor]:
        """_upload, as the tables' device twins."""
        blob, where = self._upload(tables, dev)
        return [blob[o:o + t.numel() * t.element_size()].view(t.dtype).view(t.shape) for t, o in zip(tables, where)]

    def _ingest_stage(self, specs: Sequence["_ClipSpec"], offsets: Sequence[int], dev: torch.device):
        """Brings a group of clips within reach of one wt_ingest: the resampled lengths (int32), the code spans (int64 {frames,
        offset}) and the CPU clips go up with ONE copy (_upload); clips on the GPU stay where they are.  Returns
        (descriptors, device workspace of wt_ingest, lengths on the GPU, spans on the GPU, what must stay alive)."""
        spans = [v for sp, off in zip(specs, offsets) for v in (self._arch.frames(sp.n_out), int(off))]
        tables = [torch.tensor([sp.n_out for sp in specs], dtype=torch.int32), torch.tensor(spans, dtype=torch.int64)]
        on_host = [sp.clip.device.type == "cpu" for sp in specs]
        for sp, host in zip(specs, on_host):
            if host:
                tables.append(sp.clip)
            elif sp.clip.device != dev:
                raise RuntimeError(f"a clip is on {sp.clip.device} but the model is on {dev}")
        blob, offs = self._upload(tables, dev)
        base, at = blob.data_ptr(), iter(offs[2:])
        where = [base + next(at) if host else None for host in on_host]
        return (*self._ingest_descs(specs, where, dev), blob[:4 * len(specs)].view(torch.int32),
                blob[offs[1]:offs[1] + 16 * len(specs)].view(torch.int64), (blob, [sp.clip for sp in specs]))

    def _ingest_descs(self, specs: Sequence["_ClipSpec"], where: Sequence[Optional[int]], dev: torch.device):
        """(descriptors, device workspace) of one wt_ingest over specs.  where[j] is None for a clip read where it lies (sp.clip
        on the GPU, with its strides), or the GPU address at which its samples lie contiguous in sp.clip's shape and type: its
        place in an uploaded blob, a segment of a 1-D row (an address, not a view: hundreds of segments pay for every view)."""
        from . import audio
        descs = (_capi.WtIngestClip * len(specs))()
        handles: Dict[int, ctypes.c_void_p] = {}
        codec_rate = self.codec_rate
        last = None
        for j, (sp, address) in enumerate(zip(specs, where)):
            if sp is last and address is not None and where[j - 1] is not None:
                descs[j] = descs[j - 1]                      # a run of ONE spec (a recording's full segments): the same descriptor
                descs[j].src = address                       # at another address, copied instead of filled field by field
                continue
            d, c, last = descs[j], sp.clip, sp
            d.src = c.data_ptr() if address is None else address
            d.dtype = _capi.WT_INGEST_I16 if c.dtype == torch.int16 else _capi.WT_INGEST_F32
            d.channels, d.n_in, d.n_out = sp.channels, sp.n_in, sp.n_out
            if c.dim() == 1:
                d.ch_stride, d.sample_stride = 0, 1 if address is not None else c.stride(0)
            else:
                st = c.stride() if address is None else (c.shape[1], 1)
                d.ch_stride, d.sample_stride = (st[1], st[0]) if sp.channels_last else (st[0], st[1])
            if sp.rate not in handles:
                handles[sp.rate] = audio.resampler(sp.rate, codec_rate, dev.index)
            d.resampler = handles[sp.rate]
        return descs, torch.empty(max(int(lib.wt_ingest_workspace_bytes(len(specs))), 8), dtype=torch.uint8, device=dev)

    def _ingest_rows(self, specs: Sequence["_ClipSpec"], dev: torch.device) -> torch.Tensor:
        """The clips at the codec rate as the rows of one new (len(specs), longest) fp32 tensor: one upload, one wt_ingest."""
        T_pad = max(sp.n_out for sp in specs)
        descs, ws, _lengths, _spans, _alive = self._ingest_stage(specs, [0] * len(specs), dev)
        rows = torch.empty((len(specs), T_pad), dtype=torch.float32, device=dev)
        check(lib.wt_ingest(descs, len(specs), T_pad, _ptr(rows), _ptr(ws), _stream_ptr(dev)), "wt_ingest")
        return rows

    def _run_encode_codes_mixed(self, specs: Sequence["_ClipSpec"], T_pad: int, flat: torch.Tensor, offsets: Sequence[int],
                                n_q: Optional[int] = None, norm=None):
        """One group of encode_codes_many: one upload, one wt_ingest into the plan's staging tensor, one wt_encode_mixed (no
        feature buffer unless the plan is graph-replayed), one wt_codes_unpack into flat at the clips' offsets.  Returns True, or
        None when the encoder is off the route a mixed-length plan takes (_route_ok).  n_q: residual VQ (_encode_ingested).
        norm: (mode, gain, sink, ceiling) of a call with normalize=...: the ingested rows are normalised in place in front of the
        encode (one wt_normalize_rows) and sink(offsets, scales) receives the group's divisors; ceiling: max_true_peak_db or None."""
        dev = self._ensure_engine()
        if not self._route_ok(_capi.WT_PLAN_ENCODE):          # (before anything is uploaded; checked again on every attempt below)
            return None
        descs, ws, lengths, spans, _alive = self._ingest_stage(specs, offsets, dev)
        rows_norm = norm and (norm[0], norm[1], [sp.n_out for sp in specs], lambda scales: norm[2](offsets, scales), norm[3])
        return self._encode_ingested(descs, ws, len(specs), T_pad, lengths, spans, flat, dev, n_q, rows_norm)

    def _encode_ingested(self, descs, ws: torch.Tensor, B: int, T_pad: int, lengths: Optional[torch.Tensor], spans: torch.Tensor,
                         flat: torch.Tensor, dev: torch.device, n_q: Optional[int] = None, norm=None):
        """The launches of a group whose wt_ingest descriptors, lengths (int32) and code spans (int64 {frames, offset}) are on
        hand, the latter two on the GPU: one wt_ingest into the plan's staging tensor, one encode without a feature tensor, one
        wt_codes_unpack into flat.  lengths=None: B clips of T_pad samples each on the plain encode plan (encode_codes' own: same
        recording, same staging buffers).  True, or None off the mixed route (a uniform batch then goes clip by clip as well).
        n_q: the encode is residual VQ with n_q codebooks (WT_PLAN_FLAG_RVQ), flat is [n_q][sum L_i] and every plane is handed
        out by a wt_codes_unpack of its own.
        norm: (mode, gain, samples per row, sink, ceiling): behind the ingest, one wt_normalize_rows divides every row by its own
        level in place (audio.normalize_rows, ceiling its max_true_peak_db) and sink(scales) receives the divisors (B,)."""
        def fill_wav(buf: torch.Tensor):
            check(lib.wt_ingest(descs, B, T_pad, _ptr(buf), _ptr(ws), _stream_ptr(dev)), "wt_ingest")
            if norm is not None:
                from . import audio
                norm[3](audio.normalize_rows(buf, norm[2], norm[0], norm[1], sample_rate=self.codec_rate, max_true_peak_db=norm[4]))

        if n_q is not None:
            if lengths is None:
                thunk = lambda: self._encode_rvq(B, T_pad, fill_wav, n_q, self._graph_flags(B), dev)
            else:
                thunk = lambda: self._encode_rvq_mixed(B, T_pad, fill_wav, lengths, n_q, dev)
            res = self._guarded_mixed(_capi.WT_PLAN_ENCODE, B, thunk, dev)
            if res is None:
                return None
            for k in range(n_q):
                check(lib.wt_codes_unpack(_ptr(res[0][k]), B, self._arch.frames(T_pad), _ptr(spans), _ptr(flat[k]), flat[k].numel(),
                                          _stream_ptr(dev)), "wt_codes_unpack")
            return True
        if lengths is None:
            thunk = lambda: self._encode(B, T_pad, fill_wav, self._graph_flags(B), dev, want_emb=False, want_feats=False)
        else:
            thunk = lambda: self._encode_mixed(B, T_pad, fill_wav, lengths, dev, want_feats=False)
        res = self._guarded_mixed(_capi.WT_PLAN_ENCODE, B, thunk, dev)
        if res is None:
            return None
        check(lib.wt_codes_unpack(_ptr(res[1]), B, self._arch.frames(T_pad), _ptr(spans), _ptr(flat), flat.numel(), _stream_ptr(dev)),
              "wt_codes_unpack")
        return True

    def _encode_codes_solo(self, specs: Sequence["_ClipSpec"], flat: torch.Tensor, offsets: Sequence[int], n_q: Optional[int] = None,
                           norm=None):
        """Clips that run one at a time (shorter than a mixed-length plan takes, or the encoder off its shipped route): ingested
        together like a group, at most MAX_GROUP per launch, then encode_codes per clip (with n_q: into the planes of flat)."""
        from .mixed_length import MAX_GROUP
        dev = self._ensure_engine()
        for c0 in range(0, len(specs), MAX_GROUP):
            part, offs = specs[c0:c0 + MAX_GROUP], offsets[c0:c0 + MAX_GROUP]
            wav = self._ingest_rows(part, dev)
            if norm is not None:                             # (as _run_encode_codes_mixed: in place, behind the ingest)
                from . import audio
                norm[2](offs, audio.normalize_rows(wav, [sp.n_out for sp in part], norm[0], norm[1], sample_rate=self.codec_rate,
                                                   max_true_peak_db=norm[3]))
            for j, (sp, off) in enumerate(zip(part, offs)):
                if n_q is not None:
                    codes = self.encode_codes(wav[j:j + 1, :sp.n_out], n_q=n_q)
                    flat[:, off:off + codes.shape[-1]].copy_(codes[:, 0, :])
                    continue
                codes = self.encode_codes(wav[j:j + 1, :sp.n_out])
                flat[off:off + codes.shape[-1]].copy_(codes.view(-1))

    def _clip_specs(self, who: str, clips: Sequence[torch.Tensor], sample_rates, channels_last: bool) -> List["_ClipSpec"]:
        """The clips of encode_codes_many / encode_codes_segmented_many, checked: ValueError for anything wt_ingest would refuse."""
        from . import audio
        clips = list(clips)
        codec_rate = self.codec_rate
        rates = self._rates(who, sample_rates, len(clips))
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
                          bandwidth_id=None, n_q: Optional[int] = None, normalize: Optional[str] = None, target_db: float = 0.0,
                          return_scales: bool = False, target_lufs: Optional[float] = None, *,
                          max_true_peak_db: Optional[float] = None):
        """Tokenise a set of clips straight from PCM.  clips[i] is (T,), (C, T) or, with channels_last, (T, C), C in {1, 2}, fp32
        or int16 (scaled by 1 / 32768), on the CPU or on the model's device; sample_rates is one rate or one per clip (default:
        the codec rate).  Returns [codes (1, 1, L_i)] in input order, views into one flat int64 tensor, L_i =
        arch.frames(ceil(24000 * T_i / rate_i)); packed=True returns (that flat tensor [sum L_i], offsets [n + 1] on the CPU).
        Clip i's codes are the bits of encode_infer(audio.convert_audio(clip i as planar fp32, rate_i, 24000, 1)[0], ...)[1].
        Per group of encode_infer_many's grouping (on the resampled lengths): one upload of the group's CPU clips, one ragged
        ingest launch, one mixed-length encode without a feature tensor, one launch that hands out the codes.  Clips under the
        mixed-length plans' minimum, and every clip while the encoder is off its shipped route, are ingested the same way and
        encoded one at a time; a model whose first encoder ratio (the last of arch.ratios) is neither 2 nor 4 is always off it
        (_route_ok: no stage-1 kernel that takes per-clip lengths).  Argument errors raise ValueError before any GPU work.
        n_q, an int in [1, num_quantizers]: residual VQ with the first n_q codebooks, clip i's codes the bits of
        encode_codes(..., n_q=n_q).  Returns [codes (n_q, 1, L_i)], views into one flat tensor laid out [n_q][sum L_i];
        packed=True returns (that tensor as (n_q, sum L_i), offsets).  Per group one ingest, one mixed-length residual VQ encode
        and n_q launches that hand out the codes, one per plane.
        normalize="peak" or "rms": every clip is level-normalised between the ingest and the encode, on its mono row at the codec
        rate (one wt_normalize_rows per group, in place): clip i's codes are the bits of encode_infer(audio.normalize(
        audio.convert_audio(clip i, rate_i, 24000, 1)[0], normalize, target_db)[0])[1].  "peak" is extract_features.py:27-28 (the
        codec was trained on peak-normalised audio), target_db its peak target in dB (peak mode only); "rms" Encodec's frame
        normalisation.  The order is the reference scripts': convert first, normalise second; sox's `norm` runs before the
        resampling and a peak moves under resampling, so parity with sox is not claimed.  return_scales=True (with normalize)
        appends the divisors, (n,) fp32 on the model's device, to the result: (codes list, scales) or (flat, offsets, scales);
        decode_pcm_many(scales=...) multiplies them back in.  A target_db without "peak", an unknown mode and return_scales
        without normalize raise ValueError before any GPU work.
        normalize="lufs" (target_lufs, default -23): every clip is brought to that integrated loudness (ITU-R BS.1770-4, measured
        on its mono row at the codec rate; one wt_normalize_rows_lufs per group): clip i's codes are the bits of encode_infer(
        audio.normalize(converted clip i, "lufs", target_lufs=...)[0])[1], its scale that call's.  A clip without a loudness
        (under 400 ms after conversion, silent, all under -70 LUFS) is tokenised as it is with scale 1; there is no limiter.  A
        target_lufs without "lufs" raises ValueError like the rest.
        max_true_peak_db (dBTP, with "lufs" only): the gain is bounded so that no clip's true peak (ITU-R BS.1770-4 Annex 2, on the
        same row) exceeds it: one wt_normalize_rows_lufs_tp per group, clip i's codes and scale those of audio.normalize(converted
        clip i, "lufs", target_lufs=..., max_true_peak_db=...).  Given without "lufs", or no finite number: ValueError."""
        from . import audio
        from .mixed_length import group_clips
        self._check_bandwidth(bandwidth_id)
        norm = audio.normalize_args("encode_codes_many", normalize, target_db, target_lufs)
        ceiling = audio.ceiling_arg("encode_codes_many", normalize, max_true_peak_db)
        if return_scales and norm is None:
            raise ValueError("encode_codes_many: return_scales needs normalize")
        if n_q is not None:
            n_q = self._check_n_q("encode_codes_many", n_q)
        specs = self._clip_specs("encode_codes_many", clips, sample_rates, channels_last)
        offsets = [0]
        frames = self._arch.frames
        for sp in specs:
            offsets.append(offsets[-1] + frames(sp.n_out))
        flat = torch.empty(offsets[-1] if n_q is None else (n_q, offsets[-1]), dtype=torch.int64, device=self._device())
        rvq = () if n_q is None else (n_q,)       # (n_q=None: today's calls, argument for argument)
        parts: Dict[int, Tuple[List[int], torch.Tensor]] = {}    # a group's first code offset -> (its clips' offsets, their divisors)
        kw = {} if norm is None else {"norm": (*norm, lambda offs, sc: parts.__setitem__(offs[0], (list(offs), sc)), ceiling)}
        self._run_groups_of(specs, offsets, *group_clips([sp.n_out for sp in specs], self._arch.hop),
                            lambda T_pad, part, offs: self._run_encode_codes_mixed(part, T_pad, flat, offs, *rvq, **kw),
                            lambda part, offs: self._encode_codes_solo(part, flat, offs, *rvq, **kw))
        extra = (self._gather_scales(parts, offsets[:-1]),) if return_scales else ()
        if packed:
            return (flat, torch.tensor(offsets, dtype=torch.int64), *extra)
        if n_q is not None:
            out = [flat[:, offsets[i]:offsets[i + 1]].unsqueeze(1) for i in range(len(specs))]
        else:
            out = [flat[offsets[i]:offsets[i + 1]].view(1, 1, -1) for i in range(len(specs))]
        return (out, *extra) if extra else out

    def _gather_scales(self, parts, keys: Sequence[int]) -> torch.Tensor:
        """The divisors of a normalising call in input order: parts maps anything to (the keys of a launch's rows, their divisors
        (rows,) on the GPU), keys[i] is the key of input i.  One concatenation and one gather (an index table goes up)."""
        dev = self._device()
        if not keys:
            return torch.empty(0, dtype=torch.float32, device=dev)
        where = {k: j for j, k in enumerate(k for ks, _sc in parts.values() for k in ks)}
        cat = torch.cat([sc for _ks, sc in parts.values()])
        return cat[torch.tensor([where[k] for k in keys], dtype=torch.int64).to(dev)]

    # -- long recordings in overlapping segments (segmented.py): tokenise ---------------------------------------------------------
    @torch.inference_mode()
    def encode_codes_segmented_many(self, clips: Sequence[torch.Tensor], segment_length: int, stride: int, sample_rates=None,
                                    channels_last: bool = False, bandwidth_id=None, normalize: Optional[str] = None,
                                    target_db: float = 0.0, target_lufs: Optional[float] = None, *,
                                    max_true_peak_db: Optional[float] = None):
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
        segment beyond 12 000 frames, an ISTFT head with padding="center") raise ValueError before any GPU work.
        normalize="peak" or "rms" (target_db with "peak"): every segment is normalised on its own after the cut, as
        EncodecModel._encode_frame does with "rms" (encoder/model.py:147-165), one wt_normalize_rows per call between its ingest
        and its encode: segment i's codes are the bits of encode_codes(audio.normalize(W[None, off_i:off_i + len_i], normalize,
        target_db)[0]), and the divisors are kept as SegmentedCodes.scales, (n_segments,) fp32 on the model's device, for
        decode_pcm_segmented to multiply back in.  normalize="lufs" (target_lufs) brings every segment to that integrated
        loudness in the same place; a segment under 400 ms (the last cut of a recording may be) passes as it is with scale 1;
        max_true_peak_db (with "lufs" only) bounds every segment's gain by its own true peak, as in encode_codes_many."""
        from . import audio
        from .mixed_length import MAX_GROUP, group_clips
        from .segmented import SegmentedCodes, check_geometry, segment_plan
        who = "encode_codes_segmented_many"
        self._check_bandwidth(bandwidth_id)
        norm = audio.normalize_args(who, normalize, target_db, target_lufs)
        ceiling = audio.ceiling_arg(who, normalize, max_true_peak_db)
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
        # every recording at the codec rate: W of recording r is rows[r]
        rows: List[torch.Tensor] = []
        c0 = 0
        while c0 < len(specs):
            c1, T_pad = c0, 0
            while c1 < len(specs) and c1 - c0 < MAX_GROUP and (c1 == c0 or (c1 - c0 + 1) * max(T_pad, specs[c1].n_out) <= 1 << 28):
                T_pad = max(T_pad, specs[c1].n_out)
                c1 += 1
            rows += self._ingest_rows(specs[c0:c1], dev)
            c0 = c1
        base = [row.data_ptr() for row in rows]
        # a segment of n samples as a clip: fp32 mono at the codec rate (the sample type alone is read from the clip: any row serves)
        spec = {n: _ClipSpec(rows[0], 1, n, False, self.codec_rate, n) for n in set(seg_len)}
        on_route = self._route_ok(_capi.WT_PLAN_ENCODE)
        full = [k for k in range(len(seg_len)) if seg_len[k] == S] if on_route else []
        tails = [k for k in range(len(seg_len)) if seg_len[k] != S] if on_route else []
        groups, short = group_clips([seg_len[k] for k in tails], self._arch.hop)
        solo = [tails[i] for i in short] if on_route else list(range(len(seg_len)))
        # the calls: (padded length or 0 for a uniform batch, segments); ONE upload carries all their lengths and spans
        calls = [(0, full[i:i + MAX_GROUP]) for i in range(0, len(full), MAX_GROUP)]
        calls += [(T_pad, [tails[i] for i in idx]) for T_pad, idx in groups]
        tables, frames = [], self._arch.frames
        for _T_pad, ks in calls:
            tables.append(torch.tensor([seg_len[k] for k in ks], dtype=torch.int32))
            tables.append(torch.tensor([v for k in ks for v in (frames(seg_len[k]), seg_code[k])], dtype=torch.int64))
        on_gpu = self._upload_tables(tables, dev)
        tables_of = iter(zip(on_gpu[0::2], on_gpu[1::2]))            # (_run_groups runs the calls in this order, each once)

        parts: Dict[int, Tuple[List[int], torch.Tensor]] = {}    # a call's first segment -> (its segments, their divisors)

        def run_call(T_pad, ks):         # the segments are wt_ingest clips at equal rates: addresses in the rows
            lengths, spans = next(tables_of)
            descs, ws = self._ingest_descs([spec[seg_len[k]] for k in ks], [base[seg_rec[k]] + 4 * seg_off[k] for k in ks], dev)
            uniform = not T_pad and not self._segment_uniform_mixed
            kw = {} if norm is None else {"norm": (*norm, [seg_len[k] for k in ks], lambda sc: parts.__setitem__(ks[0], (list(ks), sc)), ceiling)}
            return self._encode_ingested(descs, ws, len(ks), T_pad or S, None if uniform else lengths, spans, flat, dev, **kw)

        def run_solo(ks):
            for k in ks:
                seg = rows[seg_rec[k]][None, seg_off[k]:seg_off[k] + seg_len[k]]
                if norm is None:
                    codes = self.encode_codes(seg)
                else:
                    codes, sc = self.encode_codes(seg, normalize=normalize, target_db=target_db, return_scales=True, target_lufs=target_lufs,
                                                  max_true_peak_db=ceiling)
                    parts[k] = ([k], sc)
                flat[seg_code[k]:seg_code[k] + codes.shape[-1]].copy_(codes.view(-1))

        self._run_groups(calls, solo, run_call, run_solo)
        if norm is None:
            return [SegmentedCodes(flat[bounds[r]:bounds[r + 1]], rec_offsets[r], sp.n_out, S, stride) for r, sp in enumerate(specs)]
        scales = self._gather_scales(parts, list(range(len(seg_len))))
        first = [0]
        for offs in rec_offsets:
            first.append(first[-1] + len(offs) - 1)
        return [SegmentedCodes(flat[bounds[r]:bounds[r + 1]], rec_offsets[r], sp.n_out, S, stride, scales[first[r]:first[r + 1]])
                for r, sp in enumerate(specs)]

    @torch.inference_mode()
    def encode_codes_segmented(self, clip: torch.Tensor, segment_length: int, stride: int, sample_rate: Optional[int] = None,
                               channels_last: bool = False, bandwidth_id=None, normalize: Optional[str] = None, target_db: float = 0.0,
                               target_lufs: Optional[float] = None, *, max_true_peak_db: Optional[float] = None):
        """encode_codes_segmented_many for one recording: its segmented.SegmentedCodes."""
        return self.encode_codes_segmented_many([clip], segment_length, stride, sample_rates=sample_rate, channels_last=channels_last,
                                                bandwidth_id=bandwidth_id, normalize=normalize, target_db=target_db, target_lufs=target_lufs,
                                                max_true_peak_db=max_true_peak_db)[0]

    def _run_decode_mixed(self, feats: List[torch.Tensor], L_pad: int, bw: int, dev: Optional[torch.device] = None):
        """One mixed-length decode call (WT_PLAN_DECODE_MIXED) on clips (512, L_i) of 1 <= L_i <= L_pad frames: returns the
        waveforms (B, wave_len(L_pad)), clip j's own samples first and zeros behind them, or None when the current flags or
        fp32 sites keep the decoder off the route a mixed-length plan takes (_route_ok; the caller then decodes
        the clips one at a time).  Any other refusal of the plan raises."""
        dev = dev if dev is not None else self._ensure_engine()
        B = len(feats)
        lengths = [int(f.shape[1]) for f in feats]
        if min(lengths) < 1 or max(lengths) > L_pad:
            raise ValueError("every clip needs between 1 and L_pad frames")

        def fill_feats(buf: torch.Tensor):
            for j, f in enumerate(feats):
                buf[j, :, :lengths[j]].copy_(f)

        res = self._guarded_mixed(_capi.WT_PLAN_DECODE_MIXED, B, lambda: self._decode_mixed(B, L_pad, fill_feats, lengths, bw, dev), dev)
        return res and res[0]

    def _waves_many(self, clips: Sequence[torch.Tensor], run_mixed, run_one) -> List[torch.Tensor]:
        """decode_many and decode_codes_many behind their argument checks: clips[i] is (rows, L_i); run_mixed(clips of a group,
        L_pad) returns the group's padded waveforms or None, run_one(clip) a clip's own (1, wave_len(L_i))."""
        out: List[Optional[torch.Tensor]] = [None] * len(clips)

        def run_group(L_pad, idx):
            wav = run_mixed([clips[i] for i in idx], L_pad)
            if wav is None:
                return None
            for j, i in enumerate(idx):
                out[i] = wav[j:j + 1, :self._wave_len(int(clips[i].shape[1]))].clone()
            return True

        def run_solo(idx):
            for i in idx:
                out[i] = run_one(clips[i])

        self._run_groups(*self._decode_groups([int(c.shape[1]) for c in clips]), run_group, run_solo)
        return out  # type: ignore[return-value]

    @torch.inference_mode()
    def decode_many(self, features: Sequence[torch.Tensor], bandwidth_id=None) -> List[torch.Tensor]:
        """decode over clips of different lengths (the reference's infer.py loop, one call per file) in a few batched calls:
        features[i] is (512, L_i) or (1, 512, L_i) with L_i >= 1; returns [(1, wave_len(L_i))] in input order, each the same
        bits as decode(features[i][None], bandwidth_id=...), whatever the other clips and the grouping.  Clips are sorted by
        length and grouped (mixed_length.group_frames: at most 64 per call and at most MAX_SCORE_CELLS attention score cells,
        padded to a coarse bucket so that calls share plans and graphs).  A clip that forms a group alone, and every clip while
        the decoder runs off its shipped route (set_gemm_precision("f32"), an fp32 decoder site after a range fallback, the
        unfused debug plans), goes through decode."""
        dev = self._ensure_engine()
        bw = self._bandwidth_index(bandwidth_id)
        feats: List[torch.Tensor] = []
        for f in features:
            if isinstance(f, torch.Tensor) and f.dim() == 3 and f.shape[0] == 1:
                f = f[0]
            if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[0] != self._arch.input_channels or f.shape[1] < 1:
                raise ValueError("decode_many takes a sequence of tensors (512, L) or (1, 512, L) with L >= 1")
            feats.append(self._as_input(f, dev))
        return self._waves_many(feats, lambda fs, L_pad: self._run_decode_mixed(fs, L_pad, bw, dev),
                                lambda f: self.decode(f[None], bandwidth_id=bw))

    @torch.inference_mode()
    def _run_decode_codes_mixed(self, codes_list: List[torch.Tensor], L_pad: int, bw: int, dev: Optional[torch.device] = None,
                                borrow: bool = False):
        """One mixed-length decode-from-codes call (WT_PLAN_DECODE_CODES_MIXED) on clips (K, L_i) int64 of 1 <= L_i <= L_pad
        frames, the counterpart of _run_decode_mixed: returns the waveforms (B, wave_len(L_pad)), clip j's own samples first and
        zeros behind them, or None when the decoder is off the route a mixed-length plan takes (_route_ok).  What
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

        res = self._guarded_mixed(_capi.WT_PLAN_DECODE_CODES_MIXED, B,
                                  lambda: self._decode_codes_mixed(K, B, L_pad, fill_codes, lengths, bw, dev, borrow), dev)
        if res is None:
            return None
        self._codes_checked(dev)
        return res[0]

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
        bw = self._bandwidth_index(bandwidth_id)
        return self._waves_many(self._codes_clips(codes, "decode_codes_many"),
                                lambda cs, L_pad: self._run_decode_codes_mixed(cs, L_pad, bw),
                                lambda c: self.decode_codes(c, bandwidth_id=bw))

    def round_trip_mel_distance(self, wavs: Sequence[torch.Tensor], *, n_q: Optional[int] = None, bandwidth_id=None, **kw) -> torch.Tensor:
        """How well the codec gives a set of clips back, as the reference's val/mel_loss per clip: wavs is a list of 1-D fp32 clips
        at the codec rate on the model's device; returns (n,) fp32.  It is encode_codes_many -> decode_codes_many -> each output
        cropped to its input's length -> metrics.mel_distance_many(outputs, wavs, **kw), and nothing else; n_q and bandwidth_id
        go to the two codec calls (the decoder needs a bandwidth_id, as in decode), kw (sample_rate, n_fft, hop_length, n_mels) to
        the metric."""
        from . import metrics
        wavs = list(wavs)
        if not wavs:
            return torch.zeros(0, dtype=torch.float32, device=self._ensure_engine())
        codes = self.encode_codes_many(wavs, bandwidth_id=bandwidth_id, n_q=n_q)
        outs = self.decode_codes_many(codes, bandwidth_id=bandwidth_id)
        return metrics.mel_distance_many([o[0, :w.shape[-1]] for o, w in zip(outs, wavs)], wavs, **kw)

    def round_trip_stoi(self, wavs: Sequence[torch.Tensor], *, n_q: Optional[int] = None, bandwidth_id=None,
                        extended: bool = False) -> torch.Tensor:
        """How intelligible the codec gives a set of clips back: STOI (extended=True: ESTOI) per clip, (n,) fp32.  wavs is a list of
        1-D fp32 clips at the codec rate, 24 kHz, on the model's device.  It is round_trip_mel_distance with the other metric:
        encode_codes_many -> decode_codes_many -> each output cropped to its input's length -> metrics.stoi_many(wavs, outputs,
        sample_rate=24000, extended=extended), and nothing else."""
        from . import metrics
        wavs = list(wavs)
        if not wavs:
            return torch.zeros(0, dtype=torch.float32, device=self._ensure_engine())
        codes = self.encode_codes_many(wavs, bandwidth_id=bandwidth_id, n_q=n_q)
        outs = self.decode_codes_many(codes, bandwidth_id=bandwidth_id)
        return metrics.stoi_many(wavs, [o[0, :w.shape[-1]] for o, w in zip(outs, wavs)], sample_rate=24000, extended=extended)

    def round_trip_periodicity(self, wavs: Sequence[torch.Tensor], *, n_q: Optional[int] = None, bandwidth_id=None, **kw) -> torch.Tensor:
        """How the codec keeps pitch and voicing: per clip the reference's periodicity RMSE, pitch RMSE in cents and voiced / unvoiced
        F1 (metrics.periodicity_metrics_many: YIN, not the reference's CREPE), (n, 3) fp32.  wavs is a list of 1-D fp32 clips at the
        codec rate, 24 kHz, on the model's device.  It is encode_codes_many -> decode_codes_many -> each output cropped to its
        input's length -> metrics.periodicity_metrics_many(wavs, outputs, sample_rate=24000, **kw), and nothing else; kw carries
        threshold, silence_threshold and unvoiced_threshold."""
        from . import metrics
        wavs = list(wavs)
        if not wavs:
            return torch.zeros((0, 3), dtype=torch.float32, device=self._ensure_engine())
        codes = self.encode_codes_many(wavs, bandwidth_id=bandwidth_id, n_q=n_q)
        outs = self.decode_codes_many(codes, bandwidth_id=bandwidth_id)
        return metrics.periodicity_metrics_many(wavs, [o[0, :w.shape[-1]] for o, w in zip(outs, wavs)], sample_rate=24000, **kw)

    def round_trip_report(self, wavs: Sequence[torch.Tensor], n_q: Optional[int] = None, bandwidth_id=None,
                          extended: bool = False, periodicity: bool = False) -> Dict[str, torch.Tensor]:
        """Every measure of how the codec gives a set of clips back from one pass through the codec: one encode_codes_many, one
        decode_codes_many, each output cropped to its input's length, then the metrics on those outputs.  wavs is a list of 1-D fp32
        clips at the codec rate, 24 kHz, on the model's device.  Returns a dict of (n,) fp32 tensors: mel_distance, stoi, estoi (with
        extended=True), stft_distance, si_sdr, snr; each carries the bits of the separate call (round_trip_mel_distance,
        round_trip_stoi, metrics.stft_distance_many, si_sdr_many, snr_many) on the same outputs.  periodicity=True adds
        periodicity_loss, pitch_loss and vuv_f1 behind them, the columns of round_trip_periodicity bit for bit."""
        from . import metrics
        wavs = list(wavs)
        if not wavs:
            empty = torch.zeros(0, dtype=torch.float32, device=self._ensure_engine())
            keys = ["mel_distance", "stoi"] + (["estoi"] if extended else []) + ["stft_distance", "si_sdr", "snr"]
            keys += ["periodicity_loss", "pitch_loss", "vuv_f1"] if periodicity else []
            return {k: empty.clone() for k in keys}
        codes = self.encode_codes_many(wavs, bandwidth_id=bandwidth_id, n_q=n_q)
        outs = self.decode_codes_many(codes, bandwidth_id=bandwidth_id)
        outs = [o[0, :w.shape[-1]] for o, w in zip(outs, wavs)]
        report = {"mel_distance": metrics.mel_distance_many(outs, wavs),
                  "stoi": metrics.stoi_many(wavs, outs, sample_rate=24000, extended=False)}
        if extended:
            report["estoi"] = metrics.stoi_many(wavs, outs, sample_rate=24000, extended=True)
        report["stft_distance"] = metrics.stft_distance_many(outs, wavs)
        both = metrics.wavedist_many(outs, wavs, who="round_trip_report")
        report["si_sdr"], report["snr"] = both[:, 0], both[:, 1]
        if periodicity:
            three = metrics.periodicity_metrics_many(wavs, outs, sample_rate=24000)
            report["periodicity_loss"], report["pitch_loss"], report["vuv_f1"] = three[:, 0], three[:, 1], three[:, 2]
        return report

    # -- synthesise straight to PCM: decode from codes -> ragged emit (resample, channels, layout, sample type) into one tensor -----
    def _emit_format(self, who: str, channels, dtype, limit, n: int) -> Tuple[List[int], Tuple[torch.dtype, float]]:
        """(channels per clip, (dtype, limit)) of decode_pcm / decode_pcm_many over n clips, checked: ValueError for anything
        wt_emit would refuse."""
        if dtype not in (torch.float32, torch.int16):
            raise ValueError(who + ": dtype must be torch.float32 or torch.int16")
        channels = self._per_clip(channels, n, who + ": one channel count, or one per clip")
        if any(isinstance(c, bool) or c not in (1, 2) for c in channels):
            raise ValueError(who + ": channels must be 1 or 2")
        limit = float(limit)
        if not 0.0 < limit <= 1.0:
            raise ValueError(who + ": limit must be in (0, 1]")
        return [int(c) for c in channels], (dtype, limit)

    def _scale_rows(self, rows: Sequence[torch.Tensor], lens: Sequence[int], scales: torch.Tensor, dev: torch.device):
        """One wt_scale_rows: rows[j][:lens[j]] *= scales[j] in place; rows are contiguous fp32 rows on dev, scales (len(rows),)
        fp32 there.  The row pointers and lengths go up in one copy."""
        assert scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == len(rows) and scales.device == dev
        assert all(r.dtype == torch.float32 and r.stride(-1) == 1 and r.shape[-1] >= n >= 1 for r, n in zip(rows, lens))
        table, lengths = self._upload_tables([torch.tensor([r.data_ptr() for r in rows], dtype=torch.int64),
                                              torch.tensor(list(lens), dtype=torch.int64)], dev)
        with torch.cuda.device(dev):
            check(lib.wt_scale_rows(_ptr(table), _ptr(lengths), _ptr(scales), len(rows), max(lens), _stream_ptr(dev)), "wt_scale_rows")

    def _check_scales(self, who: str, scales, n: int) -> Optional[torch.Tensor]:
        """The scales argument of decode_pcm / decode_pcm_many, checked: None, or (n,) floating point, as fp32 on the model's device."""
        if scales is None:
            return None
        if not isinstance(scales, torch.Tensor) or not scales.is_floating_point() or scales.shape != (n,):
            raise ValueError(who + ": scales must be a floating-point tensor with one entry per clip")
        return scales.to(device=self._device(), dtype=torch.float32).contiguous()

    def _emit_rows(self, rows: Sequence[torch.Tensor], specs: Sequence["_PcmSpec"], flat: torch.Tensor, offsets: Sequence[int],
                   fmt: Tuple[torch.dtype, float], channels_last: bool, dev: torch.device, rescale: bool = False):
        """One wt_emit: rows[j], a contiguous fp32 row of at least specs[j].n_in samples at the codec rate on dev, goes to
        flat[offsets[j]:] at the clip's rate in the layout (channels, n_out) or, with channels_last, (n_out, channels).
        rescale: wt_emit_rescaled instead (two launches): every clip times min(limit / its peak, 1) in place of the clamp."""
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
        if rescale:                     # (the peaks lie in the workspace: one per call)
            ws = torch.empty(int(lib.wt_emit_rescaled_workspace_bytes(B)), dtype=torch.uint8, device=dev)
            check(lib.wt_emit_rescaled(descs, B, _ptr(ws), _stream_ptr(dev)), "wt_emit_rescaled")
            return
        if B <= 64:
            ws = self._emit_ws
            if ws is None or ws.device != dev:
                ws = self._emit_ws = torch.empty(max(int(lib.wt_emit_workspace_bytes(64)), 8), dtype=torch.uint8, device=dev)
        else:
            ws = torch.empty(int(lib.wt_emit_workspace_bytes(B)), dtype=torch.uint8, device=dev)
        check(lib.wt_emit(descs, B, _ptr(ws), _stream_ptr(dev)), "wt_emit")

    def _run_decode_pcm_mixed(self, specs: Sequence["_PcmSpec"], L_pad: int, bw: int, flat: torch.Tensor, offsets: Sequence[int],
                              fmt: Tuple[torch.dtype, float], channels_last: bool, rescale: bool = False, scales_of=None):
        """One group of decode_pcm_many: one wt_decode_codes_mixed, one wt_emit from the plan's output rows into flat at the
        clips' offsets.  Returns True, or None when the decoder is off the route a mixed-length plan takes.  scales_of(offsets):
        the clips' scales, multiplied into the rows in front of the emit (wt_scale_rows); rescale as in _emit_rows."""
        wav = self._run_decode_codes_mixed([sp.codes for sp in specs], L_pad, bw, borrow=True)
        if wav is None:
            return None
        if scales_of is not None:
            self._scale_rows(list(wav), [sp.n_in for sp in specs], scales_of(offsets), wav.device)
        self._emit_rows(list(wav), specs, flat, offsets, fmt, channels_last, wav.device, rescale)
        return True

    def _decode_pcm_solo(self, specs: Sequence["_PcmSpec"], bw: int, flat: torch.Tensor, offsets: Sequence[int],
                         fmt: Tuple[torch.dtype, float], channels_last: bool, rescale: bool = False, scales_of=None):
        """Clips that are decoded one at a time (a group of one, a 'center' clip under two frames, every clip while the decoder
        is off its mixed route): decode_codes per clip, then one wt_emit for the lot, at most MAX_GROUP clips per launch."""
        from .mixed_length import MAX_GROUP
        for c0 in range(0, len(specs), MAX_GROUP):
            part, offs = specs[c0:c0 + MAX_GROUP], offsets[c0:c0 + MAX_GROUP]
            rows = [self.decode_codes(sp.codes, bandwidth_id=bw)[0] for sp in part]
            if scales_of is not None:
                self._scale_rows(rows, [sp.n_in for sp in part], scales_of(offs), rows[0].device)
            self._emit_rows(rows, part, flat, offs, fmt, channels_last, rows[0].device, rescale)

    @torch.inference_mode()
    def decode_pcm_many(self, codes: Sequence[torch.Tensor], sample_rates=None, channels=1, dtype: torch.dtype = torch.int16,
                        channels_last: bool = False, limit: float = 0.99, packed: bool = False, device=None, bandwidth_id=None,
                        rescale: bool = False, scales: Optional[torch.Tensor] = None):
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
        reports it.  Argument errors raise ValueError before any GPU work.
        rescale=True: save_audio's rescale (encoder/utils.py:95-103) per clip instead of the clamp: the emit is wt_emit_rescaled
        (two launches per group), clip i the bits of audio.to_pcm16(R_i, rescale=True, limit=limit) (int16) or of R_i times
        min(limit / max |R_i|, 1) (fp32).  scales: (n,) from encode_codes_many(return_scales=True): every decoded row is
        multiplied by its clip's scale in front of the emit (one wt_scale_rows per group)."""
        from . import audio
        who = "decode_pcm_many"
        bw = self._bandwidth_index(bandwidth_id)
        clips = self._codes_clips(codes, who)
        scales = self._check_scales(who, scales, len(clips))
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
        kw = {"rescale": True} if rescale else {}
        if scales is not None:                               # (a clip is known by its offset in flat: every clip has samples)
            index = {off: i for i, off in enumerate(offsets[:-1])}
            kw["scales_of"] = lambda offs: scales[torch.tensor([index[o] for o in offs], dtype=torch.int64).to(scales.device)]
        self._run_groups_of(specs, offsets, *self._decode_groups([sp.frames for sp in specs]),
                            lambda L_pad, part, offs: self._run_decode_pcm_mixed(part, L_pad, bw, flat, offs, fmt, channels_last, **kw),
                            lambda part, offs: self._decode_pcm_solo(part, bw, flat, offs, fmt, channels_last, **kw))
        return self._pcm_result(flat, offsets, specs, packed, to_host, channels_last)

    def _pcm_rates_device(self, who: str, n: int, sample_rates, device) -> Tuple[List[int], bool]:
        """(rate per clip, whether the result goes to the host) of decode_pcm_many / decode_pcm_segmented_many, checked."""
        rates = self._rates(who, sample_rates, n)
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
                                  limit: float = 0.99, packed: bool = False, device=None, bandwidth_id=None, rescale: bool = False):
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
        ValueError before any GPU work.
        A recording with scales (encode_codes_segmented(normalize=...)) has segment i's decoded samples multiplied by scales[i]
        in front of the cross-fade, EncodecModel._decode_frame's `out * scale` (one wt_scale_rows over all such segments): X is
        then audio.linear_overlap_add([decode_codes(c_i)[..., :len_i] * scales[i] for i], stride), bit for bit.  rescale as in
        decode_pcm_many, on the cross-faded recording."""
        from . import audio
        from .mixed_length import MAX_GROUP, MAX_SCORE_CELLS, score_cells
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
        on_route = self._route_ok(_capi.WT_PLAN_DECODE_CODES)
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
        uniform = []                                                 # (frames, segments) per decode_codes batch
        for L, ks in by_frames.items():
            per_call = max(1, min(MAX_GROUP, MAX_SCORE_CELLS // score_cells(1, L)))
            uniform += [(L, ks[c0:c0 + per_call]) for c0 in range(0, len(ks), per_call)]
        seg_codes = lambda k: codes[items[k][0]][items[k][2]:items[k][2] + items[k][3]].view(1, -1)

        def keep(part, wav):
            for j, k in enumerate(part):
                rows[items[k][0]][items[k][1]] = wav[j]
            return True

        def run_uniform(L, part):
            B = len(part)
            runs: List[List[int]] = []                               # consecutive segments of one recording are one slice of its codes
            for k in part:
                r, _i, o, _L = items[k]
                if runs and runs[-1][0] == r and runs[-1][2] == o:
                    runs[-1][2] = o + L
                else:
                    runs.append([r, o, o + L])
            pieces = [codes[r][a:b] for r, a, b in runs]
            batch = (pieces[0] if len(pieces) == 1 else torch.cat(pieces)).view(1, B, L)
            res = self._guarded_mixed(_capi.WT_PLAN_DECODE_CODES, B,
                                      lambda: self._decode_codes(batch, bw, self._decode_flags(self._graph_flags(B)), dev), dev)
            return res and keep(part, res[0])

        def run_tails(L_pad, part):
            wav = self._run_decode_codes_mixed([seg_codes(k) for k in part], L_pad, bw, dev)
            return None if wav is None else keep(part, wav)

        def run_solo(ks):
            for k in ks:
                rows[items[k][0]][items[k][1]] = self.decode_codes(seg_codes(k), bandwidth_id=bw)[0]

        self._run_groups(uniform, [], run_uniform, solo.extend)      # (refused batches only JOIN solo here: it runs once, below)
        if uniform:
            self._codes_checked(dev)
        groups, lone = self._decode_groups([items[k][3] for k in rest])
        self._run_groups([(L_pad, [rest[i] for i in idx]) for L_pad, idx in groups], solo + [rest[i] for i in lone], run_tails, run_solo)
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
        scaled = [r for r, sc in enumerate(segs) if sc.scales is not None]
        if scaled:                                                   # _decode_frame's out * scale, on the rows, before the cross-fade
            self._scale_rows([row for r in scaled for row in rows[r]], [n for r in scaled for n in geo[r][1]],
                             torch.cat([segs[r].scales.to(device=dev, dtype=torch.float32).reshape(-1) for r in scaled]), dev)
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
                            [offsets[r] for r in part], fmt, channels_last, dev, bool(rescale))
        return self._pcm_result(flat, offsets, specs, packed, to_host, channels_last)

    @torch.inference_mode()
    def decode_pcm_segmented(self, seg, sample_rate: Optional[int] = None, channels: int = 1, dtype: torch.dtype = torch.int16,
                             channels_last: bool = False, limit: float = 0.99, packed: bool = False, device=None, bandwidth_id=None,
                             rescale: bool = False):
        """decode_pcm_segmented_many for one recording: (channels, n_out) or, with channels_last, (n_out, channels); packed=True
        returns the flat tensor and its offsets."""
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)):
            raise ValueError("decode_pcm_segmented: channels must be 1 or 2")
        out = self.decode_pcm_segmented_many([seg], sample_rates=sample_rate, channels=channels, dtype=dtype, channels_last=channels_last,
                                             limit=limit, packed=packed, device=device, bandwidth_id=bandwidth_id, rescale=rescale)
        return out if packed else out[0]

