"""The contract all plans share: the caller owns the workspace and the library may assume nothing about its contents.

Every runnable case of tests/ws_ref.MATRIX is created with wt_plan_create_ex and run through its C entry point on a workspace in
each state of ws_ref.STATES; against the call on a zero-filled workspace (the baseline) every other state must give

  - return code 0, and after a synchronise wt_plan_status, wt_model_status, wt_plan_range_sites, wt_model_take_bad_codes all 0
  - every output the SAME WORDS as the baseline (integer views) and finite; that covers the documented fill past each clip of a
    mixed-length plan, which is part of its outputs
  - the 4 KiB bands on either side of the workspace and of every output intact
  - WT_PLAN_FLAG_RANGE_REPORT: every reported maximum the same word
  - WT_PLAN_FLAG_KEEP_STAGES: every named buffer the same words, not only the outputs, with three exact exceptions that are
    checked inside the case (_unwritten): regions that plan.cpp leaves unwritten by design must still hold the poison, word
    for word, and everything outside them must be the baseline's words

WT_PLAN_FLAG_GRAPH plans make three calls per state (direct, record + replay, replay) with the poison written again before each.
There is no tolerance in this file.  The tests of one case come in the order history, finite, ones: the mildest state first
(pytest -x then stops at the mildest dependence).  On a mismatch ws_ref.blame() names the buffers whose poisoning alone changes
an output, and the message carries them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import ws_ref as W
from tests.util import manifest

pytestmark = pytest.mark.gpu

_MODELS = {}
_BASE = {}           # case id -> baseline outputs (CPU).  A plan with its workspace and arenas lives for one test only
COMPARED = {}        # case id -> set of states compared with the baseline
REACHED = set()      # kernel forms the runs reached (test_every_case_and_form_was_reached)
GN_SLAB_MAX = 256    # ops.hip launch_gn_apply / launch_gn_stats: the one-pass GroupNorm forms up to this many frames (dim 768)
SOFTMAX_REG_MAX = 2048       # ops.hip launch_softmax: the register forms up to this row pitch, softmax_kernel beyond


def _lib():
    from wavtokenizer_amd import _capi
    return _capi.lib


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _model(name):
    """hop600 / hop320 on the fixtures' synthetic weights with the SEANet decoder; hop600q3: hop600 with three codebooks."""
    import dataclasses
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth
    if name not in _MODELS:
        arch = dataclasses.replace(NAMED_ARCHS["hop600"], num_quantizers=3) if name == "hop600q3" else NAMED_ARCHS[name]
        sd = synth.make_state_dict(arch, seed=manifest()["weight_seed"], with_seanet_decoder=True)
        m = WavTokenizer.from_arch(arch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        m = m.eval().to("cuda")
        m._ensure_engine()
        _MODELS[name] = m
    return _MODELS[name]


def _err():
    msg = _lib().wt_last_error()
    return msg.decode() if msg else ""


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _inputs(c: W.Case, which: str):
    """The call's inputs on the CPU.  "main": the call every state repeats; "other": the call that precedes it in the `history`
    state (another seed at three times the scale, another bandwidth_id, another K and the other length set where they exist)."""
    from wavtokenizer_amd import synth
    main = which == "main"
    seed = (1000 * c.B + c.frames) * 2 + (0 if main else 1)
    scale = 1.0 if main else 3.0
    gen = torch.Generator().manual_seed(seed)
    out = {"bw": 0 if main else 2, "K": c.K if main else 1}
    if c.kind == W.ENCODE:
        out["in"] = torch.from_numpy(synth.make_clips(c.B, c.length, seed=seed)) * scale
    elif c.kind in W.CODES_KINDS:
        bins = _model(c.arch).arch.vq_bins
        codes = torch.zeros(c.K, c.B, c.length, dtype=torch.int64)
        codes[:out["K"]] = torch.from_numpy(np.random.default_rng(seed).integers(0, bins, size=(out["K"], c.B, c.length)))
        out["in"] = codes
    elif c.kind in (W.DECODE, W.DECODE_MIXED, W.SEANET_DECODER):
        out["in"] = torch.randn(c.B, 512, c.length, generator=gen) * 0.5 * scale
    elif c.kind == W.HEAD:
        out["in"] = torch.randn(c.B, c.length, _model(c.arch).arch.dim, generator=gen) * scale
    else:
        out["in"] = torch.randn(c.B, c.length, 512, generator=gen) * 0.5 * scale
    if c.lengths:
        out["lengths"] = torch.tensor(c.lengths if main else c.other_lengths, dtype=torch.int32)
    return out


# ------------------------------------------------------------------------------------------------------------- live plan
class _Live:
    """One plan of the matrix with its workspace, inputs and outputs in arenas of their own."""

    def __init__(self, c: W.Case):
        from wavtokenizer_amd import _capi
        lib, dev = _lib(), _dev()
        self.c, self.m = c, _model(c.arch)
        self.model = self.m._engine.model
        self.plan = ctypes.c_void_p()
        rc = lib.wt_plan_create_ex(self.model, c.kind, c.B, c.length, c.flags, W.site_mask(c.sites), ctypes.byref(self.plan))
        assert rc == 0 and self.plan, (c.id, rc, _err())
        self.nbytes = lib.wt_plan_workspace_bytes(self.plan)
        assert self.nbytes >= 256 and self.nbytes % 256 == 0, self.nbytes
        self.ws = W.arena(self.nbytes, dev)
        self.regions, self.fmt, i = [], {}, 0
        while True:
            s = ctypes.c_char_p()
            if lib.wt_plan_buffer_name(self.plan, i, ctypes.byref(s)) != 0:
                break
            off, n, fmt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
            assert lib.wt_plan_buffer_info(self.plan, s.value, ctypes.byref(off), ctypes.byref(n), ctypes.byref(fmt)) == 0
            assert off.value % 256 == 0 and off.value + 4 * n.value <= self.nbytes, (c.id, s.value, off.value, n.value, self.nbytes)
            self.regions.append((s.value.decode(), off.value, 4 * n.value))
            self.fmt[s.value.decode()] = fmt.value
            i += 1
        self.steps = []
        for i in range(lib.wt_plan_num_steps(self.plan)):
            s = ctypes.c_char_p()
            assert lib.wt_plan_step_name(self.plan, i, ctypes.byref(s)) == 0
            self.steps.append(s.value.decode())
        self.launches = lib.wt_plan_num_launches(self.plan)
        self.graph = bool(c.flags & W.GRAPH)
        # inputs (one arena each, written in place so that a recorded graph keeps serving) and outputs
        main = _inputs(c, "main")
        self.a_in, self.t_in = W.arena_like(main["in"], dev)
        self.a_len = self.t_len = None
        if c.lengths:
            self.a_len, self.t_len = W.arena_like(main["lengths"], dev)
        arch, L = self.m.arch, c.frames
        shapes = {}
        if c.kind == W.ENCODE:
            shapes["codes"] = ((1, c.B, L), torch.int64)
            if c.outs == "all":
                shapes["features"] = ((c.B, 512, L), torch.float32)
                shapes["emb_out"] = ((c.B, 512, L), torch.float32)
        elif c.kind in W.DECODE_KINDS:
            shapes["wav"] = ((c.B, self.m._wave_len(L)), torch.float32)
            if c.kind in (W.DECODE, W.DECODE_CODES):
                shapes["backbone_out"] = ((c.B, L, arch.dim), torch.float32)
        elif c.kind == W.HEAD:
            shapes["wav"] = ((c.B, self.m._wave_len(L)), torch.float32)
        elif c.kind == W.SEANET_DECODER:
            shapes["wav"] = ((c.B, L * lib.wt_model_hop(self.model)), torch.float32)
        else:
            shapes["y"] = ((c.B, L, 512), torch.float32)
        self.a_out, self.t_out = {}, {}
        for k, (shape, dtype) in shapes.items():
            self.a_out[k] = W.arena(int(np.prod(shape)) * (8 if dtype == torch.int64 else 4), dev)
            self.t_out[k] = self.a_out[k].view(dtype, shape)
        self.bw, self.K = 0, c.K
        self._note_forms()

    def _note_forms(self):
        """The forms this plan reaches, from its buffer and step names (plan.cpp names a buffer only where a kernel uses it)."""
        lib, c = _lib(), self.c
        names = {n for n, _o, _b in self.regions}
        lstm = [n for n in names if n.endswith(".hx")]
        if any(n.endswith(".state") for n in names):
            if lstm and lib.wt_model_persistent_lstm(self.model):
                REACHED.add("lstm persistent, at most 64 clips" if c.B <= 64 else "lstm persistent, more than 64 clips")
            else:
                assert self.launches >= c.frames + 2, (c.id, self.launches)          # L + 1 step launches and the state fill
                REACHED.add("lstm step kernel, fp32" if (c.flags & W.FP32_GEMM or c.sites == "enc") else "lstm step kernel, split f16")
        if "bb.attn.s" in names:
            s32 = "bb.attn.p" in names
            assert self.fmt["bb.attn.vt"] == (1 if s32 else 0), (c.id, self.fmt["bb.attn.vt"])
            REACHED.add(("softmax into S32 probabilities" if s32 else "softmax in place") + (", mixed lengths" if c.mixed else ""))
            REACHED.add("attention on S32 operands" if s32 else "attention on fp32 operands")
            if (c.frames + 31) // 32 * 32 > SOFTMAX_REG_MAX:
                REACHED.add("softmax read-modify-write kernel" + (", S32 probabilities" if s32 else ", in place"))
            if c.frames > GN_SLAB_MAX:
                REACHED.add("GroupNorm chunked form")
        if "mix.geom" in names:
            REACHED.add("encoder geometry table")
        if "code_rows" in self.steps:
            REACHED.add("code_rows")

    def close(self):
        if self.plan:
            _lib().wt_plan_destroy(self.plan)
            self.plan = ctypes.c_void_p()
        self.ws = self.a_in = self.t_in = self.a_len = self.t_len = None
        self.a_out, self.t_out = {}, {}

    def load(self, which):
        inp = _inputs(self.c, which)
        self.t_in.copy_(inp["in"])
        if self.t_len is not None:
            self.t_len.copy_(inp["lengths"])
        self.bw, self.K = inp["bw"], inp["K"]

    def invoke(self, ws_ptr=None):
        """One call of the plan's entry point on the current stream; returns its return code."""
        lib, c = _lib(), self.c
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        ws = ctypes.c_void_p(self.ws.ptr if ws_ptr is None else ws_ptr)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        o, x, ln = self.t_out, p(self.t_in), p(self.t_len)
        if c.kind == W.ENCODE and c.flags & W.MIXED_LENGTH:
            return lib.wt_encode_mixed(self.plan, x, ln, p(o.get("features")), p(o["codes"]), p(o.get("emb_out")), ws, st)
        if c.kind == W.ENCODE:
            return lib.wt_encode(self.plan, x, p(o.get("features")), p(o["codes"]), p(o.get("emb_out")), ws, st)
        if c.kind == W.DECODE:
            return lib.wt_decode(self.plan, x, self.bw, p(o["wav"]), p(o["backbone_out"]), ws, st)
        if c.kind == W.DECODE_MIXED:
            return lib.wt_decode_mixed(self.plan, x, ln, self.bw, p(o["wav"]), ws, st)
        if c.kind == W.DECODE_CODES:
            return lib.wt_decode_codes(self.plan, x, self.K, self.bw, p(o["wav"]), p(o["backbone_out"]), ws, st)
        if c.kind == W.DECODE_CODES_MIXED:
            return lib.wt_decode_codes_mixed(self.plan, x, self.K, ln, self.bw, p(o["wav"]), ws, st)
        if c.kind == W.HEAD:
            return lib.wt_head(self.plan, x, p(o["wav"]), ws, st)
        if c.kind == W.SEANET_DECODER:
            return lib.wt_seanet_decode(self.plan, x, p(o["wav"]), ws, st)
        return lib.wt_unit_run(self.plan, x, p(o["y"]), ws, st)

    def clean(self, what, arenas=()):
        """After a synchronise: nothing reported anywhere, every band intact."""
        lib = _lib()
        bits, sites = ctypes.c_int32(-1), ctypes.c_uint64(1)
        assert lib.wt_plan_status(self.plan, ctypes.byref(bits), 1) == 0 and bits.value == 0, (what, "wt_plan_status", bits.value)
        assert lib.wt_model_status(self.model, ctypes.byref(bits), 1) == 0 and bits.value == 0, (what, "wt_model_status", bits.value)
        assert lib.wt_plan_range_sites(self.plan, ctypes.byref(sites), 1) == 0 and sites.value == 0, (what, "wt_plan_range_sites", sites.value)
        assert lib.wt_model_take_bad_codes(self.model) == 0, (what, "wt_model_take_bad_codes")
        for name, a in [("workspace", self.ws), ("input", self.a_in)] + list(self.a_out.items()) + list(arenas):
            assert a.bands_intact(), f"{what}: a guard band of {name} was written"

    def call(self, what, ws=None):
        """Poisons the outputs, makes one call, synchronises, checks that it was clean; returns everything it left behind (CPU)."""
        for t in self.a_out.values():
            W.fill(t.payload, "ones")
        ws = ws or self.ws
        rc = self.invoke(ws.ptr)
        torch.cuda.synchronize()
        assert rc == 0, (what, rc, _err())
        self.clean(what, [("workspace", ws)])
        got = {k: t.cpu().clone() for k, t in self.t_out.items()}
        if self.c.flags & W.RANGE_REPORT:
            got["range report"] = self.range_report(what)
        if self.c.flags & W.KEEP_STAGES:
            for name, off, nb in self.regions:
                got["buffer " + name] = ws.payload[off: off + nb].view(torch.int32).cpu().clone()
        return got

    def range_report(self, what):
        lib, vals, i = _lib(), [], 0
        while True:
            v = ctypes.c_float()
            if lib.wt_plan_range_report(self.plan, i, None, None, ctypes.byref(v)) != 0:
                break
            vals.append(v.value)
            i += 1
        assert vals, (what, "a range-report plan without entries")
        return torch.tensor(vals, dtype=torch.float32)

    def unwritten(self, name):
        """The words of a kept buffer that no step of this plan writes, as a mask over its int32 words, or None.  From plan.cpp:
          bb.attn.s   with bb.attn.p present (attention on S32 operands): the score GEMM stores four columns at a time, so it
                      writes columns [0, L4) of the pitch Lp, L4 = L rounded up to 4; softmax masks everything from L on before
                      any use and writes the probabilities, pads as zeros, into bb.attn.p.  Columns [L4, Lp) are excused.  On
                      fp32 operands softmax writes the pads of bb.attn.s itself: nothing is excused
          X.state     with X.hx present and the persistent kernel in use: the launch-per-step kernel's state, there for the fallback
          bb.gn_part  at L <= 256: only the chunked GroupNorm of longer clips writes and reads it"""
        c = self.c
        names = {n for n, _o, _b in self.regions}
        nwords = {n: nb // 4 for n, _o, nb in self.regions}[name]
        L, Lp = c.frames, (c.frames + 31) // 32 * 32
        L4 = (L + 3) // 4 * 4
        if name == "bb.attn.s" and "bb.attn.p" in names and Lp > L4:
            assert nwords == c.B * L * Lp, (c.id, nwords)
            m = torch.zeros(c.B * L, Lp, dtype=torch.bool)
            m[:, L4:] = True
            return m.reshape(-1)
        if name.endswith(".state") and name[:-6] + ".hx" in names and _lib().wt_model_persistent_lstm(self.model):
            return torch.ones(nwords, dtype=torch.bool)
        if name == "bb.gn_part" and L <= GN_SLAB_MAX:
            return torch.ones(nwords, dtype=torch.bool)
        return None

    def run(self, prepare, what, which="main", ws=None):
        """prepare(payload) writes the workspace, then the call(s): three on a graph plan, prepared again before each; every
        call's results must be the first's.  Returns the first call's."""
        self.load(which)
        first = None
        for rep in range(3 if self.graph else 1):
            prepare((ws or self.ws).payload)
            got = self.call(f"{what}, call {rep + 1}", ws)
            if first is None:
                first = got
            else:
                bad = _mismatches(first, got)
                assert not bad, f"{what}: call {rep + 1} differs from call 1: {bad}"
        return first


def _mismatches(base, got, poison_word=None, lv=None):
    """{output: description} of what differs.  With a poison word and the plan: in a kept buffer ("buffer <name>") the region
    that the plan leaves unwritten (_Live.unwritten) must hold the poison in every word and the baseline zero; every word
    outside it must be the baseline's."""
    out = {}
    for k, b in base.items():
        g = got[k]
        if g.shape == b.shape and torch.equal(W.words(g), W.words(b)):
            continue
        if k.startswith("buffer ") and poison_word is not None and lv is not None and g.shape == b.shape:
            m = lv.unwritten(k[7:])
            if m is not None and bool((g[m] == poison_word).all()) and bool((b[m] == 0).all()) and torch.equal(g[~m], b[~m]):
                continue
        out[k] = W.describe_difference(b, g) if g.shape == b.shape else f"shape {tuple(g.shape)} for {tuple(b.shape)}"
    return out


POISON_WORD = {"finite": W.FINITE_WORD, "ones": -1, "history": None}


def _zero_run(lv):
    """The call on a zero-filled workspace: every float output finite, and on a graph plan the recording made."""
    c = lv.c
    base = lv.run(lambda p: W.fill(p, "zero"), f"{c.id} [zero]")
    for k, t in base.items():
        if t.is_floating_point() and not k.startswith("buffer "):
            assert bool(torch.isfinite(t).all()), f"{c.id} [zero]: {k} is not finite"
    if c.kind == W.ENCODE:
        v = base["codes"]
        assert int(v.min()) >= -1 and int(v.max()) < lv.m.arch.vq_bins, (c.id, int(v.min()), int(v.max()))
    if lv.graph:
        assert _lib().wt_plan_graph_replays(lv.plan) == 2, (c.id, _lib().wt_plan_graph_replays(lv.plan))
    if c.id in _BASE:
        bad = _mismatches(_BASE[c.id], base)
        assert not bad, f"{c.id} [zero]: a second plan of the case differs from the first: {bad}"
    else:
        _BASE[c.id] = base
    return _BASE[c.id]


def _baseline(c):
    if c.id not in _BASE:
        lv = _Live(c)
        try:
            _zero_run(lv)
        finally:
            lv.close()
    return _BASE[c.id]


def _check_state(c, state):
    """One state of one case on a plan of its own (plan, workspace and arenas are released when the test ends, so the file's
    peak is one case's buffers beside the baselines kept on the host)."""
    lv = _Live(c)
    try:
        what = f"{c.id} [{state}]"
        if state == "history":
            # the workspace as the baseline call left it, then a successful call on other inputs, then the call itself
            base = _zero_run(lv)
            lv.run(lambda p: None, what + " the call before", which="other")
            prepare = lambda p: None
        else:
            base = _baseline(c)
            prepare = lambda p: W.fill(p, state)
        got = lv.run(prepare, what)
        bad = _mismatches(base, got, POISON_WORD[state], lv)
        if bad:
            outs = {k: v for k, v in base.items() if k in lv.t_out}
            poison = "ones" if state == "history" else state

            def rerun(prep):
                return {k: v for k, v in lv.run(prep, what + " blame").items() if k in outs}
            guilty = W.blame(rerun, lv.regions, outs, lv.nbytes, poison)
            if not guilty and poison != "ones":          # (a finite poison times a zero elsewhere is still zero; a NaN is not)
                guilty = W.blame(rerun, lv.regions, outs, lv.nbytes, "ones")
            pytest.fail(f"{what}: differs from the call on a zero workspace: {bad}; buffers whose poisoning alone changes an output: {guilty}")
        for k, t in got.items():
            if t.is_floating_point() and not k.startswith("buffer "):
                assert bool(torch.isfinite(t).all()), f"{what}: {k} is not finite"
        COMPARED.setdefault(c.id, set()).add(state)
    finally:
        lv.close()


_ids = lambda c: c.id


@pytest.mark.parametrize("c", W.RUNNABLE, ids=_ids)
def test_history(c):
    _check_state(c, "history")


@pytest.mark.parametrize("c", W.RUNNABLE, ids=_ids)
def test_finite(c):
    _check_state(c, "finite")


@pytest.mark.parametrize("c", W.RUNNABLE, ids=_ids)
def test_ones(c):
    _check_state(c, "ones")


# ------------------------------------------------------------------------------------------------------------- aliasing
KEPT = [c for c in W.RUNNABLE if c.flags & W.KEEP_STAGES]


@pytest.mark.parametrize("c", KEPT, ids=_ids)
def test_aliased_layout_computes_what_the_kept_layout_computes(c):
    """The test of the `used` lists: the default plan overlays buffers whose listed lifetimes do not overlap, the
    WT_PLAN_FLAG_KEEP_STAGES plan keeps every buffer apart; a step that touches a buffer it does not list shows here."""
    import dataclasses
    twin = dataclasses.replace(c, flags=c.flags & ~W.KEEP_STAGES)
    assert twin in W.RUNNABLE, twin.id
    kept, plain = _baseline(c), _baseline(twin)
    bad = _mismatches(plain, kept)
    assert not bad, f"{c.id}: the default plan and the KEEP_STAGES plan differ: {bad}"


# ------------------------------------------------------------------------------------------------- relocation, replays
MOVABLE = [c for c in W.RUNNABLE if not (c.flags & ~(W.GRAPH | W.MIXED_LENGTH)) and not c.sites and c.outs == "all"
           and (c.B, c.length) in ((2, 9000), (65, 4800), (4, 9601), (2, 50), (3, 130), (17, 40), (2, 20), (9, 7), (65, 7))]


@pytest.mark.parametrize("c", MOVABLE, ids=_ids)
def test_relocation(c):
    """One plan on workspace A, then on B (another address, all ones), then on A again: the same words each time.  A recording
    made on A is never replayed onto B: the call that changes the workspace runs directly (wt_plan_graph_replays stays)."""
    lib = _lib()
    lv = _Live(c)
    try:
        lv.load("main")
        wa, wb = lv.ws, W.arena(lv.nbytes, _dev())
        assert wa.ptr != wb.ptr
        W.fill(wa.payload, "zero")
        first = lv.call(f"{c.id} on A")
        if lv.graph:
            for _ in range(2):
                assert not _mismatches(first, lv.call(f"{c.id} on A"))
            assert lib.wt_plan_graph_replays(lv.plan) == 2
        for ws, name in ((wb, "B"), (wa, "A again"), (wb, "B again")):
            W.fill(ws.payload, "ones")
            other = wa if ws is wb else wb
            W.fill(other.payload, "finite")
            before = lib.wt_plan_graph_replays(lv.plan)
            got = lv.call(f"{c.id} on {name}", ws)
            if name == "B":              # (back on A the recording made on A may serve again; a second call on B may record anew)
                assert lib.wt_plan_graph_replays(lv.plan) == before, f"{c.id} on {name}: a recording was replayed onto another workspace"
            bad = _mismatches(first, got)
            assert not bad, f"{c.id} on {name}: {bad}"
            # the workspace the call was not given is as it was
            assert bool((other.payload.view(torch.int32) == W.FINITE_WORD).all()), f"{c.id} on {name}: the other workspace was written"
            assert other.bands_intact()
    finally:
        lv.close()


GRAPHED = [c for c in W.RUNNABLE if c.flags & W.GRAPH]


@pytest.mark.parametrize("c", GRAPHED, ids=_ids)
def test_poison_between_replays(c):
    """The fills are part of the recording: poison written between two replays of one recording changes nothing."""
    lib = _lib()
    lv = _Live(c)
    try:
        base = lv.run(lambda p: W.fill(p, "zero"), f"{c.id} [zero]")
        assert lib.wt_plan_graph_replays(lv.plan) == 2
        for n, state in enumerate(("finite", "ones", "finite", "zero", "ones")):
            W.fill(lv.ws.payload, state)
            got = lv.call(f"{c.id} replay on {state}")
            assert lib.wt_plan_graph_replays(lv.plan) == 3 + n, f"{c.id}: the call on {state} was not a replay"
            bad = _mismatches(base, got)
            assert not bad, f"{c.id}: replay on a workspace of {state}: {bad}"
    finally:
        lv.close()


# -------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("c", W.REFUSED, ids=_ids)
def test_refused_plans(c):
    from wavtokenizer_amd import _capi
    m = _model(c.arch)
    p = ctypes.c_void_p()
    rc = _lib().wt_plan_create_ex(m._engine.model, c.kind, c.B, c.length, c.flags, W.site_mask(c.sites), ctypes.byref(p))
    assert rc == _capi.WT_ERR_INVALID and not p, (c.id, rc)
    assert _err(), c.id
    bits = ctypes.c_int32(-1)
    torch.cuda.synchronize()
    assert _lib().wt_model_status(m._engine.model, ctypes.byref(bits), 0) == 0 and bits.value == 0


def _one_per_entry_point():
    seen, out = set(), []
    for c in W.RUNNABLE:
        key = (c.kind, bool(c.flags & W.MIXED_LENGTH))
        if key not in seen and c.arch == "hop600" and c.B > 1:
            seen.add(key)
            out.append(c)
    assert len(out) == 9, [c.id for c in out]
    return out


@pytest.mark.parametrize("c", _one_per_entry_point(), ids=_ids)
def test_misaligned_workspace_is_refused_before_any_launch(c):
    """Every run entry point wants the workspace on a 256-byte boundary (include/wavtokenizer_amd.h, conventions) and refuses any
    other address with WT_ERR_INVALID: nothing is launched, so neither the outputs nor the workspace change."""
    from wavtokenizer_amd import _capi
    lv = _Live(c)
    try:
        big = W.arena(lv.nbytes + 256, _dev())
        lv.load("main")
        for off in (4, 16, 128, 255):
            W.fill(big.payload, "finite")
            for a in lv.a_out.values():
                W.fill(a.payload, "ones")
            rc = lv.invoke(big.ptr + off)
            torch.cuda.synchronize()
            assert rc == _capi.WT_ERR_INVALID and "256-byte aligned" in _err(), (c.id, off, rc, _err())
            assert bool((big.payload.view(torch.int32) == W.FINITE_WORD).all()), (c.id, off)
            for k, a in lv.a_out.items():
                assert bool((a.payload == 0xFF).all()), (c.id, off, k)
        lv.clean(f"{c.id} after the refusals", [("workspace", big)])
        W.fill(lv.ws.payload, "ones")
        got = lv.call(f"{c.id} aligned")
        assert not _mismatches(_baseline(c), got)
    finally:
        lv.close()


# ------------------------------------------------------------------------------------ caller-workspace entry points
def _twice(call, ws_bytes, outs, what):
    """call(ws pointer) on a workspace of zeros, of the finite pattern and of ones: the outputs must be the same words."""
    ws = W.arena(max(ws_bytes, 4), _dev())
    base = None
    for state in ("zero", "finite", "ones"):
        W.fill(ws.payload, state)
        for t in outs.values():
            t.view(torch.uint8).fill_(0xFF) if t.dtype != torch.uint8 else t.fill_(0xFF)
        rc = call(ctypes.c_void_p(ws.ptr))
        torch.cuda.synchronize()
        assert rc == 0, (what, state, rc, _err())
        assert ws.bands_intact(), f"{what} [{state}]: a guard band of the workspace was written"
        got = {k: t.cpu().clone() for k, t in outs.items()}
        if base is None:
            base = got
        else:
            bad = {k: W.describe_difference(base[k], got[k]) for k in W.differing(base, got)}
            assert not bad, f"{what} [{state}]: {bad}"
    return base


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("kernel", ["shipped", "f32"])
def test_vq_nearest_workspace(kernel):
    lib = _lib()
    N, D, bins = 300, 512, 200
    gen = torch.Generator().manual_seed(11)
    x, embed = (torch.randn(N, D, generator=gen) * 0.7).cuda(), torch.randn(bins, D, generator=gen).cuda()
    codes = torch.empty(N, dtype=torch.int64, device="cuda")
    fn = lib.wt_vq_nearest if kernel == "shipped" else lib.wt_vq_nearest_f32
    base = _twice(lambda ws: fn(_p(x), _p(embed), N, D, bins, _p(codes), ws, None), lib.wt_vq_workspace_bytes(N, D, bins), {"codes": codes},
                  f"wt_vq_nearest {kernel}")
    assert int(base["codes"].min()) >= 0 and int(base["codes"].max()) < bins


@pytest.mark.parametrize("mode", [2, 3])
def test_linear_workspace(mode):
    """wt_linear on split-f16 operands (modes 2 and 3): the workspace holds the operands' S32 copies (M x K + N x K floats)."""
    lib = _lib()
    M, N, K = 300, 96, 160
    gen = torch.Generator().manual_seed(mode)
    x, w, b = torch.randn(M, K, generator=gen).cuda(), (torch.randn(N, K, generator=gen) / K ** 0.5).cuda(), torch.randn(N, generator=gen).cuda()
    y = torch.empty(M, N, device="cuda")
    base = _twice(lambda ws: lib.wt_linear(_p(x), _p(w), _p(b), _p(y), M, N, K, mode, ws, None), 4 * (M + N) * K + 8192, {"y": y},
                  f"wt_linear mode {mode}")
    assert bool(torch.isfinite(base["y"]).all())


def test_conv1d_s32_workspace():
    lib = _lib()
    B, T, Cin, Cout, k, stride = 2, 75, 64, 96, 4, 2
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, Cin, generator=gen).cuda()
    w, b = (torch.randn(Cout, k, Cin, generator=gen) / (Cin * k) ** 0.5).cuda(), torch.randn(Cout, generator=gen).cuda()
    y = torch.empty(B * ((T + stride - 1) // stride) * Cout, device="cuda")
    base = _twice(lambda ws: lib.wt_conv1d_s32(_p(x), _p(w), _p(b), _p(y), B, T, Cin, Cout, k, stride, 0, ws, None),
                  4 * (B * T * Cin + Cout * k * Cin) + 256, {"y": y}, "wt_conv1d_s32")
    assert bool(torch.isfinite(base["y"]).all())


def test_pcm16_rescale_workspace():
    """wt_pcm16 with rescale: the workspace holds the peak the first launch finds (one word, zeroed by the call)."""
    lib = _lib()
    n = 12345
    x = (torch.randn(n, generator=torch.Generator().manual_seed(3)) * 3.0).cuda()      # peaks far above the limit: the scale matters
    y = torch.empty(n, dtype=torch.int16, device="cuda")
    base = _twice(lambda ws: lib.wt_pcm16(_p(x), n, 1.0, 1, _p(y), ws, None), 256, {"y": y.view(torch.uint8)}, "wt_pcm16 rescale")
    assert int(base["y"].view(torch.int16).abs().max()) > 30000


def test_sconv1d_has_no_workspace():
    """wt_sconv1d (the fp32 chain) takes no workspace: its output between bands, twice, the same words."""
    lib = _lib()
    B, T, Cin, Cout, k, stride = 2, 75, 64, 96, 4, 2
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(B, T, Cin, generator=gen).cuda()
    w, b = (torch.randn(Cout, k, Cin, generator=gen) / (Cin * k) ** 0.5).cuda(), torch.randn(Cout, generator=gen).cuda()
    a = W.arena(4 * B * ((T + stride - 1) // stride) * Cout, _dev())
    got = []
    for state in ("finite", "ones"):
        W.fill(a.payload, state)
        assert lib.wt_sconv1d(_p(x), _p(w), _p(b), ctypes.c_void_p(a.ptr), B, T, Cin, Cout, k, stride, 1, 0, None) == 0, _err()
        torch.cuda.synchronize()
        assert a.bands_intact()
        got.append(a.view(torch.float32).cpu().clone())
    assert torch.equal(W.words(got[0]), W.words(got[1])) and bool(torch.isfinite(got[0]).all())


@pytest.mark.parametrize("engine", [0, 1, 2])
def test_gemm_probe_workspace(engine):
    """wt_gemm_probe on fp32 operands it splits into its workspace first (engine 0: gemm16s.hip, 1: gemm.hip, 2: the one-product
    kernel), bias epilogue, fp32 output."""
    from wavtokenizer_amd import _capi
    from tests import gemm_ref as G
    lib = _lib()
    M, N, K = 300, 96, 160
    gen = torch.Generator().manual_seed(40 + engine)
    A, Wt, bias = torch.randn(M, K, generator=gen).cuda(), (torch.randn(N, K, generator=gen) / K ** 0.5).cuda(), torch.randn(N, generator=gen).cuda()
    C = torch.empty(M, N, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _capi.WtGemmDesc()
    d.size = ctypes.sizeof(d)
    d.engine, d.epi, d.out, d.pro = engine, G.EPI_BIAS, G.OUT_F32, G.PRO_NONE
    d.M, d.N, d.K, d.nz, d.alpha = M, N, K, 1, 1.0
    d.stride, d.dil, d.taps, d.T_in, d.T_out, d.Cin = 1, 1, 1, M, M, K
    d.A, d.a_rstride, d.B, d.w_rstride, d.zW = A.data_ptr(), K, Wt.data_ptr(), K, N * K
    d.bias, d.C, d.c_rstride, d.status = bias.data_ptr(), C.data_ptr(), N, status.data_ptr()
    need = lib.wt_gemm_probe_workspace_bytes(ctypes.byref(d))
    base = _twice(lambda ws: lib.wt_gemm_probe(ctypes.byref(d), None, ws, None), max(need, 256), {"C": C}, f"wt_gemm_probe engine {engine}")
    assert bool(torch.isfinite(base["C"]).all()) and int(status[0]) == 0


@pytest.mark.parametrize("kernel", [0, 1])
def test_vq_probe_workspace(kernel):
    from wavtokenizer_amd import _capi
    lib = _lib()
    B, L, D, bins = 3, 50, 512, 200
    rows = B * L
    nparts = -(-bins // (192 if kernel == 0 else 128)) * 2          # gemm16s_vq_parts / gemm_vq_parts
    gen = torch.Generator().manual_seed(20 + kernel)
    x, embed = (torch.randn(rows, D, generator=gen) * 0.7).cuda(), torch.randn(bins, D, generator=gen).cuda()
    outs = {"codes": torch.empty(rows, dtype=torch.int64, device="cuda"), "feat": torch.empty(B, D, L, device="cuda"),
            "pval": torch.empty(rows, nparts, device="cuda"), "pidx": torch.empty(rows, nparts, dtype=torch.int32, device="cuda")}
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _capi.WtVqDesc()
    d.size = ctypes.sizeof(d)
    d.kernel, d.B, d.L, d.D, d.bins = kernel, B, L, D, bins
    d.x, d.embed, d.status = x.data_ptr(), embed.data_ptr(), status.data_ptr()
    d.codes, d.feat, d.pval, d.pidx = (outs[k].data_ptr() for k in ("codes", "feat", "pval", "pidx"))
    f = _capi.WtVqForm()
    base = _twice(lambda ws: lib.wt_vq_probe(ctypes.byref(d), ctypes.byref(f), ws, None), lib.wt_vq_workspace_bytes(rows, D, bins), outs,
                  f"wt_vq_probe kernel {kernel}")
    assert f.nparts == nparts and int(status[0]) == 0
    assert int(base["codes"].min()) >= 0 and int(base["codes"].max()) < bins and bool(torch.isfinite(base["feat"]).all())


def test_lstm_probe_workspace():
    """The LSTM probe on each of its kernels: the exchange marks (persistent) and the zeroed state (step kernels) are the
    probe's to write, as they are the plans' (plan.cpp issue_lstm)."""
    from wavtokenizer_amd import _capi
    lib, m = _lib(), _model("hop600")
    B, L, H = 9, 5, 512
    gen = torch.Generator().manual_seed(8)
    xg, x = (torch.randn(L, B, 4 * H, generator=gen) * 0.5).cuda(), (torch.randn(B, L, H, generator=gen) * 0.5).cuda()
    y = torch.empty(B, L, H, device="cuda")
    kernels = [_capi.LSTM_STEP_F16, _capi.LSTM_STEP_F32] + ([_capi.LSTM_PERSIST] if lib.wt_model_persistent_lstm(m._engine.model) else [])
    for kernel in kernels:
        d = _capi.WtLstmDesc()
        d.size, d.which, d.kernel, d.B, d.L, d.elu_out, d.out_s32 = ctypes.sizeof(d), 0, kernel, B, L, 0, 0
        d.xg, d.x, d.y, d.status = xg.data_ptr(), x.data_ptr(), y.data_ptr(), None
        need = lib.wt_lstm_probe_workspace_bytes(ctypes.byref(d))
        assert need > 0, kernel
        base = _twice(lambda ws: lib.wt_lstm_probe(m._engine.model, ctypes.byref(d), None, ws, None), need, {"y": y}, f"wt_lstm_probe kernel {kernel}")
        assert bool(torch.isfinite(base["y"]).all())
    bits = ctypes.c_int32(-1)
    assert lib.wt_model_status(m._engine.model, ctypes.byref(bits), 1) == 0 and bits.value == 0


# -------------------------------------------------------------------------------------------------------------- coverage
def test_every_case_and_form_was_reached():
    """Closing test (it reads what the tests above recorded, so it belongs to a run of the whole file): every runnable case was
    compared in every state, and the cases reached both forms of the persistent LSTM, the step kernels, both softmax forms and
    both attention operand formats, softmax's read-modify-write kernel and the chunked GroupNorm.  The LSTM form is read from
    the plan's buffers (an exchange buffer exists only where the persistent kernel is planned) and the batch size, which is
    what launch_lstm_persist chooses its instantiation by; the launch's own geometry is the business of tests/test_lstm_ops.py."""
    missing = {c.id: sorted(set(W.STATES[1:]) - COMPARED.get(c.id, set())) for c in W.RUNNABLE}
    missing = {k: v for k, v in missing.items() if v}
    assert not missing, f"{len(missing)} cases were not compared in every state, e.g. {list(missing.items())[:5]}"
    want = {"lstm step kernel, fp32", "lstm step kernel, split f16", "softmax into S32 probabilities", "softmax in place",
            "softmax into S32 probabilities, mixed lengths", "attention on S32 operands", "attention on fp32 operands",
            "encoder geometry table", "code_rows"}
    want |= {"softmax read-modify-write kernel, S32 probabilities", "softmax read-modify-write kernel, in place", "GroupNorm chunked form"}
    if _lib().wt_model_persistent_lstm(_model("hop600")._engine.model):
        want |= {"lstm persistent, at most 64 clips", "lstm persistent, more than 64 clips"}
    assert want <= REACHED, want - REACHED
