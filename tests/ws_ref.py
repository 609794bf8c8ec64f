"""Shared by tests/test_ws_checks.py (CPU) and tests/test_workspace_state.py (GPU): the workspace contract of the plans.

The caller owns the workspace and the library may assume nothing about what it holds (include/wavtokenizer_amd.h, conventions;
DESIGN.md "Workspace contract").  This module holds what both test files need and nothing that comes from a kernel:

  MATRIX            every plan the tests create: (arch, kind, B, len, flags, fp32 sites, outputs wanted, inputs) with the
                    answer wt_plan_create_ex must give (run / WT_ERR_INVALID); accepts() mirrors the library's own
                    acceptance conditions (capi.cpp wt_plan_create_ex, plan.cpp build_encode / build_decode) the way
                    tests/inv_ref.py mirrors the launchers
  STATES, fill()    the workspace states a call is made in: zero (the baseline), history, finite, ones
  Arena             a buffer between two 4 KiB guard bands
  blame()           which named buffer an output depends on

A workspace state is a byte pattern, so fill() works on uint8 tensors on any device."""
import dataclasses
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------------------ constants
# (wavtokenizer_amd/_capi.py; repeated here so that this module imports without the library)
ENCODE, DECODE, SEANET_DECODER, HEAD, UNIT_LSTM, DECODE_MIXED, DECODE_CODES, DECODE_CODES_MIXED = 0, 1, 2, 3, 4, 5, 6, 7
KIND_NAMES = {ENCODE: "encode", DECODE: "decode", SEANET_DECODER: "seanet", HEAD: "head", UNIT_LSTM: "lstm",
              DECODE_MIXED: "decode_mixed", DECODE_CODES: "decode_codes", DECODE_CODES_MIXED: "decode_codes_mixed"}
KEEP_STAGES, FP32_GEMM, STEP_LSTM, GRAPH, UNFUSED, RANGE_REPORT, MIXED_LENGTH, F16_GEMM = 1, 2, 4, 8, 16, 32, 64, 128
FLAG_NAMES = {KEEP_STAGES: "keep", FP32_GEMM: "fp32", STEP_LSTM: "step", GRAPH: "graph", UNFUSED: "unfused", RANGE_REPORT: "range",
              MIXED_LENGTH: "mixed", F16_GEMM: "f16"}
DECODE_KINDS = (DECODE, DECODE_MIXED, DECODE_CODES, DECODE_CODES_MIXED)
MIXED_DECODE_KINDS = (DECODE_MIXED, DECODE_CODES_MIXED)
CODES_KINDS = (DECODE_CODES, DECODE_CODES_MIXED)
ISTFT_KINDS = DECODE_KINDS + (HEAD,)
HOP = {"hop600": 600, "hop320": 320, "hop600q3": 600}
NUM_LAYERS = 12                      # ConvNeXt blocks of every architecture here (checked against the config in test_ws_checks)
SITE_ENC, SITE_BB_EMBED, SITE_ATTN, SITE_CNX0, SITE_HEAD = 0, 1, 4, 7, 40
MAX_FRAMES = 12000                   # capi.cpp wt_plan_create_ex
MIN_MIXED_CLIP = 1024                # plan.cpp build_encode: the fused stage-1 kernel's shortest clip
LONG_CLIP = (1, 2100)                # (B, L) of the long decode case
GRAPH_MAX_CLIPS = 16                 # ENCODE rows carry WT_PLAN_FLAG_GRAPH up to the Python layer's default graph limit; the library has none,
                                     # and the decode kinds carry the flag at every shape

STATES = ("zero", "history", "finite", "ones")
FINITE_WORD = 0x47004700             # 32 839.0 as fp32; 7.0 | 7.0 as f16 halves; a plausible positive integer
BAND = 4096
BAND_BYTE = 0xA5


def site_mask(sites: str) -> int:
    """The fp32 site mask a case names: "" (none), "enc", "attn", "all" (every decoder site, range_ref.all_decoder_sites)."""
    if sites == "":
        return 0
    if sites == "enc":
        return 1 << SITE_ENC
    if sites == "attn":
        return 1 << SITE_ATTN
    if sites == "all":
        return sum(1 << s for s in list(range(SITE_BB_EMBED, SITE_CNX0 + NUM_LAYERS)) + [SITE_HEAD])
    raise KeyError(sites)


@dataclasses.dataclass(frozen=True)
class Case:
    arch: str                        # "hop600", "hop320", "hop600q3" (hop600 with three codebooks)
    kind: int
    B: int
    length: int                      # samples (encode) or frames
    flags: int = 0
    sites: str = ""                  # site_mask()
    outs: str = "all"                # encode: "all" (features, codes, emb_out) or "codes" (features = emb_out = NULL)
    K: int = 1                       # decode from codes: codebooks the call sums
    lengths: Tuple[int, ...] = ()    # mixed plans: the call's clip lengths
    other_lengths: Tuple[int, ...] = ()      # ... and those of the call that precedes it in the `history` state
    expect: str = "run"              # or "refuse": wt_plan_create_ex returns WT_ERR_INVALID

    @property
    def id(self) -> str:
        fl = "+".join(n for b, n in FLAG_NAMES.items() if self.flags & b) or "0"
        parts = [self.arch, KIND_NAMES.get(self.kind, str(self.kind)), f"B{self.B}", f"n{self.length}", fl]
        if self.sites:
            parts.append("sites-" + self.sites)
        if self.outs != "all":
            parts.append(self.outs)
        if self.K != 1:
            parts.append(f"K{self.K}")
        if self.lengths:
            parts.append("len" + "a" if len(set(self.lengths)) == 1 else "lenb")
        if self.expect != "run":
            parts.append("refused")
        return "-".join(parts)

    @property
    def frames(self) -> int:
        h = HOP[self.arch]
        return (self.length + h - 1) // h if self.kind == ENCODE else self.length

    @property
    def mixed(self) -> bool:
        return bool(self.flags & MIXED_LENGTH) or self.kind in MIXED_DECODE_KINDS


def accepts(c: Case, padding_same: bool = True, has_seadec: bool = True) -> bool:
    """What wt_plan_create_ex answers for the case on a model whose weights fit the split-f16 range (the synthetic weights do):
    True for a plan, False for WT_ERR_INVALID.  The conditions, in the library's order: capi.cpp wt_plan_create_ex, then the
    builder of the kind (plan.cpp)."""
    mask = site_mask(c.sites)
    if c.B < 1 or c.length < 1:
        return False
    if (c.flags & MIXED_LENGTH) and c.kind != ENCODE:
        return False
    if c.flags & F16_GEMM:
        if c.kind not in DECODE_KINDS or c.flags & (FP32_GEMM | UNFUSED):
            return False
    if c.frames > MAX_FRAMES:
        return False
    if c.kind not in KIND_NAMES:
        return False
    if c.kind == ENCODE and c.B * c.length >= 2 ** 31 - 1:
        return False
    if c.kind in ISTFT_KINDS and not padding_same and c.length < 2:
        return False
    off_route = bool(c.flags & (UNFUSED | FP32_GEMM | KEEP_STAGES | RANGE_REPORT))
    if c.kind == ENCODE and c.flags & MIXED_LENGTH:
        # only the shipped split-f16 route takes lengths; the site mask's encoder bit puts the whole plan on fp32
        if off_route or (mask >> SITE_ENC) & 1 or c.length < MIN_MIXED_CLIP:
            return False
    if c.kind in CODES_KINDS and c.B * c.length >= 2 ** 31 - 1:
        return False
    if c.kind in MIXED_DECODE_KINDS and (off_route or mask):
        return False
    if c.kind == SEANET_DECODER and not has_seadec:
        return False                 # (WT_ERR_MISSING_TENSOR: no row of the matrix asks for it)
    return True


def _encode_rows(arch: str) -> List[Case]:
    rows = []
    shapes = [(1, 1927), (2, 9000), (20, 9000), (65, 4800)]      # (20, ...): persistent LSTM, whole batch; (65, ...): its BIG form
    options = [(0, ""), (STEP_LSTM, ""), (FP32_GEMM, ""), (UNFUSED | FP32_GEMM, ""), (GRAPH, ""), (KEEP_STAGES, ""), (RANGE_REPORT, ""),
               (0, "enc")]
    for B, T in shapes:
        for flags, sites in options:
            if flags & GRAPH and B > GRAPH_MAX_CLIPS:
                continue
            for outs in ("all", "codes"):
                rows.append(Case(arch, ENCODE, B, T, flags, sites, outs))
    la, lb = (9601,) * 4, (1024, 4800, 2047, 9601)
    for lengths, other in ((la, lb), (lb, la)):
        rows.append(Case(arch, ENCODE, 4, 9601, MIXED_LENGTH, lengths=lengths, other_lengths=other))
    for flags, sites, T in ((KEEP_STAGES, "", 9601), (RANGE_REPORT, "", 9601), (FP32_GEMM, "", 9601), (UNFUSED | FP32_GEMM, "", 9601),
                            (0, "enc", 9601), (0, "", 1000)):
        rows.append(Case(arch, ENCODE, 4, T, MIXED_LENGTH | flags, sites, lengths=(T,) * 4, expect="refuse"))
    rows.append(Case(arch, ENCODE, 2, 9000, F16_GEMM, expect="refuse"))
    rows.append(Case(arch, ENCODE, 0, 9000, expect="refuse"))
    rows.append(Case(arch, ENCODE, 1, HOP[arch] * MAX_FRAMES + 1, expect="refuse"))
    return rows


def _decode_rows(arch: str) -> List[Case]:
    rows = []
    shapes = [(1, 1), (2, 50), (3, 130), (17, 40)]               # (3, 130): Lp = 160, 30 pad columns; (2, 50): Lp = 64
    options = [(0, ""), (FP32_GEMM, ""), (F16_GEMM, ""), (GRAPH, ""), (KEEP_STAGES, ""), (RANGE_REPORT, ""), (0, "attn"), (0, "all")]
    for kind in (DECODE, DECODE_CODES):
        for B, L in shapes:
            for flags, sites in options:
                rows.append(Case(arch, kind, B, L, flags, sites))
        rows.append(Case(arch, kind, 2, 50, F16_GEMM | FP32_GEMM, expect="refuse"))
        rows.append(Case(arch, kind, 2, 50, F16_GEMM | UNFUSED, expect="refuse"))
        rows.append(Case(arch, kind, 2, 50, MIXED_LENGTH, expect="refuse"))
        rows.append(Case(arch, kind, 1, MAX_FRAMES + 1, expect="refuse"))
    # one long clip: the row pitch Lp = 2112 is beyond softmax's register forms (its read-modify-write kernel runs), and GroupNorm
    # takes its chunked form (L > 256), the one that writes and reads bb.gn_part
    for flags, sites in ((0, ""), (KEEP_STAGES, ""), (0, "attn")):
        rows.append(Case(arch, DECODE, LONG_CLIP[0], LONG_CLIP[1], flags, sites))
    la, lb = (130, 130, 130), (1, 77, 130)
    for kind in MIXED_DECODE_KINDS:
        for flags in (0, F16_GEMM, GRAPH):
            for lengths, other in ((la, lb), (lb, la)):
                rows.append(Case(arch, kind, 3, 130, flags, lengths=lengths, other_lengths=other))
        for flags, sites in ((KEEP_STAGES, ""), (RANGE_REPORT, ""), (FP32_GEMM, ""), (0, "attn")):
            rows.append(Case(arch, kind, 3, 130, flags, sites, lengths=la, expect="refuse"))
    for B, L in ((3, 130), (1, 1)):
        for flags in (0, KEEP_STAGES):
            rows.append(Case(arch, HEAD, B, L, flags))
    rows.append(Case(arch, HEAD, 3, 130, F16_GEMM, expect="refuse"))
    for flags in (0, KEEP_STAGES):
        rows.append(Case(arch, SEANET_DECODER, 2, 20, flags))
    for B, L in ((9, 7), (65, 7)):
        for flags in (0, STEP_LSTM, KEEP_STAGES, KEEP_STAGES | STEP_LSTM):
            rows.append(Case(arch, UNIT_LSTM, B, L, flags))
    rows.append(Case(arch, UNIT_LSTM, 9, 7, F16_GEMM, expect="refuse"))
    return rows


def _matrix() -> List[Case]:
    rows = []
    for arch in ("hop600", "hop320"):
        rows += _encode_rows(arch) + _decode_rows(arch)
    # decode from codes with K = 3 on the three-codebook architecture (the `history` call before it sums K = 1)
    for B, L in [(1, 1), (2, 50), (3, 130), (17, 40)]:
        for flags in (0, GRAPH) + ((KEEP_STAGES,) if (B, L) == (3, 130) else ()):
            rows.append(Case("hop600q3", DECODE_CODES, B, L, flags, K=3))
    for lengths, other in (((130, 130, 130), (1, 77, 130)), ((1, 77, 130), (130, 130, 130))):
        rows.append(Case("hop600q3", DECODE_CODES_MIXED, 3, 130, 0, K=3, lengths=lengths, other_lengths=other))
    return rows


MATRIX: List[Case] = _matrix()
RUNNABLE: List[Case] = [c for c in MATRIX if c.expect == "run"]
REFUSED: List[Case] = [c for c in MATRIX if c.expect == "refuse"]


# --------------------------------------------------------------------------------------------------------------- states
def fill(t: torch.Tensor, state: str) -> None:
    """Writes a poison state over a uint8 tensor whose length is a multiple of four ("history" is not a pattern: it is made by a
    call)."""
    assert t.dtype == torch.uint8 and t.numel() % 4 == 0, (t.dtype, t.numel())
    if state == "zero":
        t.zero_()
    elif state == "ones":
        t.fill_(0xFF)
    elif state == "finite":
        t.view(torch.int32).fill_(FINITE_WORD)
    else:
        raise KeyError(state)


# ---------------------------------------------------------------------------------------------------------------- arena
class Arena:
    """nbytes of payload on a 4 KiB boundary between two 4 KiB bands of 0xA5.  `payload` is a uint8 view of exactly nbytes
    (fill() wants a multiple of four); the band starts right behind the bytes asked for, so one element past the end lands
    in it."""

    def __init__(self, nbytes: int, device="cpu"):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + 2 * BAND + BAND,), BAND_BYTE, dtype=torch.uint8, device=device)
        self.start = (-(self.raw.data_ptr() + BAND)) % BAND + BAND
        self.payload = self.raw[self.start: self.start + self.nbytes]
        assert self.payload.data_ptr() % BAND == 0

    @property
    def ptr(self) -> int:
        return self.payload.data_ptr()

    def view(self, dtype, shape=None) -> torch.Tensor:
        t = self.payload.view(dtype)
        return t.view(shape) if shape is not None else t

    def bands_intact(self) -> bool:
        lo = self.raw[self.start - BAND: self.start]
        hi = self.raw[self.start + self.nbytes: self.start + self.nbytes + BAND]
        return bool((lo == BAND_BYTE).all()) and bool((hi == BAND_BYTE).all())


def arena(nbytes: int, device="cpu") -> Arena:
    return Arena(nbytes, device)


def arena_like(t: torch.Tensor, device=None) -> Tuple[Arena, torch.Tensor]:
    """An arena that holds a copy of t, and the copy as a tensor of t's type and shape."""
    a = Arena(t.numel() * t.element_size(), device if device is not None else t.device)
    v = a.view(t.dtype, t.shape)
    v.copy_(t)
    return a, v


# ---------------------------------------------------------------------------------------------------------- comparisons
def words(t: torch.Tensor) -> torch.Tensor:
    """The integer view of a tensor: NaN payloads and the sign of zero count."""
    t = t.contiguous()
    if t.dtype in (torch.float32, torch.int32):
        return t.view(torch.int32).reshape(-1)
    if t.dtype in (torch.int64, torch.uint8):
        return t.reshape(-1)
    raise TypeError(t.dtype)


def differing(base: Dict[str, torch.Tensor], got: Dict[str, torch.Tensor]) -> List[str]:
    """Names of the outputs whose words differ from the baseline's (a missing output differs)."""
    out = []
    for k, b in base.items():
        g = got.get(k)
        if g is None or g.shape != b.shape or not torch.equal(words(g), words(b)):
            out.append(k)
    return out


def describe_difference(base: torch.Tensor, got: torch.Tensor) -> str:
    wb, wg = words(base), words(got)
    idx = (wb != wg).nonzero().flatten()
    n = int(idx.numel())
    if not n:
        return "identical"
    i = int(idx[0])
    return f"{n} of {wb.numel()} words differ, first at {i}: {base.reshape(-1)[i].item()!r} -> {got.reshape(-1)[i].item()!r}"


# ---------------------------------------------------------------------------------------------------------------- blame
Region = Tuple[str, int, int]            # (name, offset in bytes, bytes)


def gap_regions(layout: Sequence[Region], nbytes: int) -> List[Tuple[int, int]]:
    """[(offset, bytes)] of the workspace that no named buffer covers (alignment gaps)."""
    covered = np.zeros(nbytes, dtype=bool)
    for _n, off, nb in layout:
        covered[off: off + nb] = True
    gaps, i = [], 0
    while i < nbytes:
        if covered[i]:
            i += 1
            continue
        j = i
        while j < nbytes and not covered[j]:
            j += 1
        gaps.append((i, j - i))
        i = j
    return gaps


def blame(run: Callable[[Callable[[torch.Tensor], None]], Dict[str, torch.Tensor]], layout: Sequence[Region], baseline: Dict[str, torch.Tensor],
          nbytes: int, state: str = "ones") -> List[str]:
    """Which buffers an output depends on.  run(prepare) makes one call on a workspace that prepare(payload) has just written and
    returns the outputs; every named buffer in turn (and the alignment gaps as one region, "<gaps>") is poisoned with `state`
    over an otherwise zero workspace.  Returns the names whose poisoning alone makes an output differ from the baseline.
    Buffers that the layout overlays share bytes, so all of the names that own the guilty bytes come back."""
    regions = [(n, [(off, nb)]) for n, off, nb in layout if nb > 0]
    gaps = gap_regions(layout, nbytes)
    if gaps:
        regions.append(("<gaps>", gaps))
    guilty = []
    for name, spans in regions:
        def prepare(payload, spans=spans):
            payload.zero_()
            for off, nb in spans:
                lo, hi = off // 4 * 4, min((off + nb + 3) // 4 * 4, payload.numel() // 4 * 4)
                fill(payload[lo:hi], state)
        if differing(baseline, run(prepare)):
            guilty.append(name)
    return guilty
