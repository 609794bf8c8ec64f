"""The helpers of tests/ws_ref.py, proven on the CPU before tests/test_workspace_state.py relies on them on the GPU.

The subject is a fake plan: a few named buffers over one workspace, laid out by the rule of wt_plan::layout() (a buffer lives
from the first to the last step that lists it, buffers whose lifetimes do not overlap may share bytes), and six numpy steps.
One variant is honest; four carry one slip each, the slips the GPU file exists to find:

  pad      reads a pad column it never wrote                     -> caught under `finite`; `ones` hides it (fmax drops NaN)
  mark     fills one word too few of a mark buffer               -> caught under `finite`; under `ones` alone the plan is right (0xFFFF is the mark)
  oob      writes one element past its workspace                 -> caught by the arena's bands, in every state
  used     omits a buffer from a step's `used` list              -> caught by comparing the aliased layout with the kept one

The run / refuse answers of the plan matrix are checked here against the mirror of the library's conditions (ws_ref.accepts);
the GPU file checks them against wt_plan_create_ex."""
import numpy as np
import pytest
import torch

from tests import ws_ref as W

MARK = 0xFFFF


class FakePlan:
    R, L, LD, N = 3, 5, 8, 6         # rows, columns, row pitch (three pad columns), mark words

    def __init__(self, slip=None, keep=False):
        self.slip, self.keep = slip, keep
        self.bufs, self.steps = {}, []
        R, LD, N = self.R, self.LD, self.N
        for name, nbytes in (("ctl", 4), ("s", 4 * R * LD), ("t", 4 * R), ("mark", 2 * N), ("acc", 4)):
            self.bufs[name] = dict(bytes=(nbytes + 15) // 16 * 16, numel_bytes=nbytes, first=10 ** 9, last=-1, off=0)
        self.step(["ctl"], self.s_clear)
        self.step(["s"], self.s_scale)
        self.step(["s", "t"], self.s_rowmax)
        self.step(["mark"], self.s_fill_marks)
        self.step(["mark", "t", "acc"], self.s_exchange)
        self.step(["ctl", "t", "acc"] + ([] if slip == "used" else ["s"]), self.s_out)
        self.layout()

    def step(self, used, fn):
        for n in used:
            b = self.bufs[n]
            b["first"], b["last"] = min(b["first"], len(self.steps)), max(b["last"], len(self.steps))
        self.steps.append(fn)

    def layout(self):
        """wt_plan::layout(): buffers in order of first use, each at the lowest offset free of every live buffer."""
        placed, self.ws_bytes = [], 0
        for name in sorted(self.bufs, key=lambda n: self.bufs[n]["first"]):
            b = self.bufs[name]
            if self.keep:
                b["last"] = 10 ** 9
            off, moved = 0, True
            while moved:
                moved = False
                for q in placed:
                    live = not (q["last"] < b["first"] or b["last"] < q["first"])
                    if live and off < q["off"] + q["bytes"] and q["off"] < off + b["bytes"]:
                        off, moved = q["off"] + q["bytes"], True
            b["off"] = off
            placed.append(b)
            self.ws_bytes = max(self.ws_bytes, off + b["bytes"])

    def regions(self):
        return [(n, b["off"], b["numel_bytes"]) for n, b in self.bufs.items()]

    def arr(self, name, dtype):
        b = self.bufs[name]
        return self.mem[self.base + b["off"]: self.base + b["off"] + b["numel_bytes"]].view(dtype)

    # ---- steps
    def s_clear(self):
        self.arr("ctl", np.int32)[:] = 0

    def s_scale(self):
        s = self.arr("s", np.float32).reshape(self.R, self.LD)
        s[:, :self.L] = 2.0 * self.x
        if self.slip != "pad":
            s[:, self.L:] = 0.0              # "pad columns stay zero"

    def s_rowmax(self):
        s = self.arr("s", np.float32).reshape(self.R, self.LD)
        self.arr("t", np.float32)[:] = np.fmax.reduce(s, axis=1)          # whole pitch; fmax drops NaN like fmaxf

    def s_fill_marks(self):
        n = self.N - 1 if self.slip == "mark" else self.N
        self.arr("mark", np.uint16)[:n] = MARK

    def s_exchange(self):
        """The data-flag exchange in program order: the reader takes a word that is not the mark for data, else waits for the writer."""
        mark, t = self.arr("mark", np.uint16), self.arr("t", np.float32)
        total = np.float32(0)
        for i in range(self.N):
            if mark[i] == MARK:
                mark[i] = np.float16(t[i % self.R] / 16 + i).view(np.uint16)
            total += np.float32(mark[i: i + 1].view(np.float16)[0])
        self.arr("acc", np.float32)[0] = total
        if self.slip == "oob":
            self.mem[self.base + self.ws_bytes: self.base + self.ws_bytes + 4].view(np.float32)[0] = total

    def s_out(self):
        s = self.arr("s", np.float32).reshape(self.R, self.LD)
        y = self.arr("t", np.float32) + self.arr("acc", np.float32)[0] + s[:, 0]
        self.y = np.where(self.arr("ctl", np.int32)[0] == 0, y, np.float32("nan")).astype(np.float32)

    def run(self, ws: W.Arena, x):
        self.mem, self.base, self.x = ws.raw.numpy(), ws.start, np.asarray(x, np.float32)
        for fn in self.steps:
            fn()
        return {"y": torch.from_numpy(self.y.copy())}


def _inputs(seed, scale=1.0):
    return (np.random.default_rng(seed).uniform(0.5, 1.5, size=(FakePlan.R, FakePlan.L)) * scale).astype(np.float32)


X, X_OTHER = _inputs(1), _inputs(2, 3.0)


def _verdict(slip):
    """{state: names of the outputs that differ from the zero baseline}, whether the bands survived every call, and the plan."""
    plan = FakePlan(slip)
    ws = W.arena(plan.ws_bytes)
    W.fill(ws.payload, "zero")
    base = plan.run(ws, X)
    intact = ws.bands_intact()
    out = {}
    for state in W.STATES[1:]:
        if state == "history":
            W.fill(ws.payload, "zero")
            plan.run(ws, X_OTHER)
        else:
            W.fill(ws.payload, state)
        got = plan.run(ws, X)
        intact = intact and ws.bands_intact()
        out[state] = W.differing(base, got)
    return out, intact, plan, base


def _blame(plan, base, state):
    ws = W.arena(plan.ws_bytes)

    def run(prepare):
        prepare(ws.payload)
        return plan.run(ws, X)
    return W.blame(run, plan.regions(), base, plan.ws_bytes, state)


def test_honest_plan_passes_every_state():
    verdict, intact, plan, base = _verdict(None)
    assert verdict == {"history": [], "finite": [], "ones": []} and intact
    assert bool(torch.isfinite(base["y"]).all())
    for state in ("finite", "ones"):
        assert _blame(plan, base, state) == []
    # and the aliased layout computes what the kept one computes
    keep = FakePlan(None, keep=True)
    wk = W.arena(keep.ws_bytes)
    W.fill(wk.payload, "zero")
    assert W.differing(base, keep.run(wk, X)) == []


def test_unwritten_pad_column_is_caught_by_finite_and_hidden_from_ones():
    verdict, intact, plan, base = _verdict("pad")
    assert verdict["finite"] == ["y"] and intact
    assert verdict["ones"] == []             # NaN pad columns fall out of the fmax: why `ones` alone is not enough
    assert _blame(plan, base, "finite") == ["s"]


def test_short_mark_fill_is_caught_by_finite_and_hidden_from_ones():
    verdict, intact, plan, base = _verdict("mark")
    assert verdict["finite"] == ["y"] and intact
    assert _blame(plan, base, "finite") == ["mark"]
    # an all-ones word is the mark itself: under `ones` the slipped plan computes what the honest plan computes, so a poison of
    # ones alone (or a comparison with a reference instead of with the zero baseline) would never show the short fill
    honest, ws, wh = FakePlan(None), W.arena(plan.ws_bytes), W.arena(plan.ws_bytes)
    W.fill(ws.payload, "ones")
    W.fill(wh.payload, "zero")
    assert W.differing(honest.run(wh, X), plan.run(ws, X)) == []
    W.fill(ws.payload, "finite")
    assert W.differing(honest.run(wh, X), plan.run(ws, X)) == ["y"]


def test_write_past_the_workspace_breaks_a_band():
    verdict, intact, _plan, _base = _verdict("oob")
    assert not intact
    assert verdict == {"history": [], "finite": [], "ones": []}          # the outputs alone would not have shown it


def test_buffer_missing_from_a_used_list_is_caught_by_the_kept_layout():
    verdict, intact, plan, base = _verdict("used")
    # the clobber is the same in every state, so the states agree with their own baseline ...
    assert verdict == {"history": [], "finite": [], "ones": []} and intact
    # ... the layout really overlays the two buffers ...
    s, mark = plan.bufs["s"], plan.bufs["mark"]
    assert s["off"] < mark["off"] + mark["bytes"] and mark["off"] < s["off"] + s["bytes"]
    # ... and the plan with every buffer kept apart computes something else
    keep = FakePlan("used", keep=True)
    wk = W.arena(keep.ws_bytes)
    W.fill(wk.payload, "zero")
    assert W.differing(base, keep.run(wk, X)) == ["y"]
    honest = FakePlan(None)
    wh = W.arena(honest.ws_bytes)
    W.fill(wh.payload, "zero")
    assert W.differing(honest.run(wh, X), keep.run(wk, X)) == []


# ------------------------------------------------------------------------------------------------------ arena and states
def test_arena_alignment_and_bands():
    for n in (4, 256, 4096, 4100, 12345 * 4):
        a = W.arena(n)
        assert a.ptr % 4096 == 0 and a.payload.numel() == n and a.bands_intact()
        a.payload.fill_(0)
        assert a.bands_intact()
        a.raw[a.start + n] = 0               # one byte past the end
        assert not a.bands_intact()
        a.raw[a.start + n] = W.BAND_BYTE
        a.raw[a.start - 1] = 0               # one byte before the start
        assert not a.bands_intact()
    t = torch.arange(12, dtype=torch.int64).reshape(3, 4)
    a, v = W.arena_like(t)
    assert torch.equal(v, t) and v.data_ptr() == a.ptr and a.bands_intact()


def test_states_are_the_documented_patterns():
    t = torch.empty(16, dtype=torch.uint8)
    W.fill(t, "finite")
    assert t.view(torch.float32).tolist() == [32839.0] * 4 and t.view(torch.float16).tolist() == [7.0] * 8
    W.fill(t, "ones")
    assert bool(torch.isnan(t.view(torch.float32)).all()) and bool(torch.isnan(t.view(torch.float16)).all())
    assert t.view(torch.int32).tolist() == [-1] * 4 and t.view(torch.int16).tolist() == [-1] * 8         # -1, and the LSTM's mark
    W.fill(t, "zero")
    assert t.tolist() == [0] * 16


def test_gap_regions_and_words():
    assert W.gap_regions([("a", 0, 10), ("b", 16, 16)], 48) == [(10, 6), (32, 16)]
    assert W.gap_regions([("a", 0, 32), ("b", 16, 32)], 48) == []
    a, b = torch.tensor([0.0, float("nan")]), torch.tensor([-0.0, float("nan")])
    assert W.differing({"x": a}, {"x": b}) == ["x"] and W.differing({"x": a}, {"x": a.clone()}) == []
    assert "1 of 2 words differ, first at 0" in W.describe_difference(a, b)


# ------------------------------------------------------------------------------------------------------------ the matrix
def test_matrix_answers_follow_the_library_conditions():
    from wavtokenizer_amd import NAMED_ARCHS
    from tests import range_ref
    for name in ("hop600", "hop320"):
        arch = NAMED_ARCHS[name]
        assert arch.hop == W.HOP[name] and arch.num_layers == W.NUM_LAYERS and arch.padding == "same"
        assert W.site_mask("all") == range_ref.all_decoder_sites(arch)
    ids = [c.id for c in W.MATRIX]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    for c in W.MATRIX:
        assert W.accepts(c) == (c.expect == "run"), c.id
        assert not (c.kind == W.ENCODE and c.flags & W.GRAPH and c.B > W.GRAPH_MAX_CLIPS), c.id
    assert len(W.RUNNABLE) + len(W.REFUSED) == len(W.MATRIX) and len(W.REFUSED) >= 30


def test_matrix_holds_the_rows_the_contract_is_tested_on():
    have = {(c.arch, c.kind, c.B, c.length, c.flags, c.sites, c.outs, c.K, c.lengths) for c in W.RUNNABLE}
    for arch in ("hop600", "hop320"):
        for B, T in ((1, 1927), (2, 9000), (20, 9000), (65, 4800)):
            for flags, sites in ((0, ""), (W.STEP_LSTM, ""), (W.FP32_GEMM, ""), (W.UNFUSED | W.FP32_GEMM, ""), (W.KEEP_STAGES, ""),
                                 (W.RANGE_REPORT, ""), (0, "enc")) + (((W.GRAPH, ""),) if B <= 16 else ()):
                for outs in ("all", "codes"):
                    assert (arch, W.ENCODE, B, T, flags, sites, outs, 1, ()) in have
        for lengths in ((9601,) * 4, (1024, 4800, 2047, 9601)):
            assert (arch, W.ENCODE, 4, 9601, W.MIXED_LENGTH, "", "all", 1, lengths) in have
        for kind in (W.DECODE, W.DECODE_CODES):
            for B, L in ((1, 1), (2, 50), (3, 130), (17, 40)):
                for flags, sites in ((0, ""), (W.FP32_GEMM, ""), (W.F16_GEMM, ""), (W.KEEP_STAGES, ""), (W.RANGE_REPORT, ""), (0, "attn"),
                                     (0, "all"), (W.GRAPH, "")):           # the graph flag at every shape, (17, 40) included
                    assert (arch, kind, B, L, flags, sites, "all", 1, ()) in have
        for kind in W.MIXED_DECODE_KINDS:
            for flags in (0, W.F16_GEMM, W.GRAPH):
                for lengths in ((130, 130, 130), (1, 77, 130)):
                    assert (arch, kind, 3, 130, flags, "", "all", 1, lengths) in have
        for row in ((W.HEAD, 3, 130, 0), (W.HEAD, 1, 1, 0), (W.SEANET_DECODER, 2, 20, 0), (W.UNIT_LSTM, 9, 7, 0), (W.UNIT_LSTM, 65, 7, 0),
                    (W.UNIT_LSTM, 9, 7, W.STEP_LSTM), (W.UNIT_LSTM, 65, 7, W.STEP_LSTM)):
            for keep in (0, W.KEEP_STAGES):     # every kind that accepts KEEP_STAGES has a kept twin (the test of the `used` lists)
                assert (arch, row[0], row[1], row[2], row[3] | keep, "", "all", 1, ()) in have
        for flags, sites in ((0, ""), (W.KEEP_STAGES, ""), (0, "attn")):
            assert (arch, W.DECODE) + W.LONG_CLIP + (flags, sites, "all", 1, ()) in have
    for B, L in ((1, 1), (2, 50), (3, 130), (17, 40)):
        for flags in (0, W.GRAPH):
            assert ("hop600q3", W.DECODE_CODES, B, L, flags, "", "all", 3, ()) in have
    assert ("hop600q3", W.DECODE_CODES, 3, 130, W.KEEP_STAGES, "", "all", 3, ()) in have
    # a kept case has its default twin
    for c in W.RUNNABLE:
        if c.flags & W.KEEP_STAGES:
            assert (c.arch, c.kind, c.B, c.length, c.flags & ~W.KEEP_STAGES, c.sites, c.outs, c.K, c.lengths) in have, c.id
    for c in W.RUNNABLE:
        if c.lengths:
            assert len(c.lengths) == c.B and len(c.other_lengths) == c.B and c.lengths != c.other_lengths, c.id
            lo = W.MIN_MIXED_CLIP if c.kind == W.ENCODE else 1
            assert all(lo <= n <= c.length for n in c.lengths + c.other_lengths), c.id


def test_constants_are_the_bindings():
    from wavtokenizer_amd import _capi as c
    assert (W.ENCODE, W.DECODE, W.SEANET_DECODER, W.HEAD, W.UNIT_LSTM, W.DECODE_MIXED, W.DECODE_CODES, W.DECODE_CODES_MIXED) == (
        c.WT_PLAN_ENCODE, c.WT_PLAN_DECODE, c.WT_PLAN_SEANET_DECODER, c.WT_PLAN_HEAD, c.WT_PLAN_UNIT_LSTM, c.WT_PLAN_DECODE_MIXED,
        c.WT_PLAN_DECODE_CODES, c.WT_PLAN_DECODE_CODES_MIXED)
    assert (W.KEEP_STAGES, W.FP32_GEMM, W.STEP_LSTM, W.GRAPH, W.UNFUSED, W.RANGE_REPORT, W.MIXED_LENGTH, W.F16_GEMM) == (
        c.WT_PLAN_FLAG_KEEP_STAGES, c.WT_PLAN_FLAG_FP32_GEMM, c.WT_PLAN_FLAG_STEP_LSTM, c.WT_PLAN_FLAG_GRAPH, c.WT_PLAN_FLAG_UNFUSED,
        c.WT_PLAN_FLAG_RANGE_REPORT, c.WT_PLAN_FLAG_MIXED_LENGTH, c.WT_PLAN_FLAG_F16_GEMM)
    assert (W.SITE_ENC, W.SITE_BB_EMBED, W.SITE_ATTN, W.SITE_CNX0, W.SITE_HEAD) == (
        c.WT_SITE_ENCODER, c.WT_SITE_BB_EMBED, c.WT_SITE_ATTN, c.WT_SITE_CNX0, c.WT_SITE_HEAD)
