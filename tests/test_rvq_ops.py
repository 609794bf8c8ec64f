"""vq_residual_kernel alone, through wt_vq_residual_probe: one round of residual VQ between two distance GEMMs.  The candidates
are built on the host, so any code can be forced.  Every output word is compared, without a tolerance: the codes against the
serial first-maximum scan of the candidates, r against numpy's float32 subtraction, the S32 form of r against wt_split_probe
op 0 on the returned r, |r|^2 against wt_op_probe(WT_OP_ROW_SUMSQ) on the returned r.  Outputs are pre-filled with NaN bits
between guard words; the status word is clear except in the one designed overflow case."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -559038737                # 0xDEADBEEF
NAN_BITS = 0x7FC00000
NO_INDEX = 0x7FFFFFFF
ROWS = [1, 3, 4, 5, 63, 64, 65, 257]
DS = [256, 512, 768]
NPARTS = [1, 2, 7, 8, 9, 44, 64, 65, 172]
BINS = [4, 100, 4096]
_EMBED = {}


class Out:
    """A device output of n 32-bit words between two guard runs, pre-filled (as tests/test_vq_ops.Out)."""

    def __init__(self, n, fill=NAN_BITS):
        self.n = n
        h = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32)
        h[GUARD:GUARD + n] = fill
        self.buf = h.cuda()
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def host(self):
        h = self.buf.cpu()
        assert bool((h[:GUARD] == SENT).all()) and bool((h[GUARD + self.n:] == SENT).all()), "guard words overwritten"
        return h[GUARD:GUARD + self.n].contiguous()


def embed_of(bins, D):
    """One seeded codebook per (bins, D), on both sides; row 1 holds zeros of both signs, row 2 large values (the overflow case)."""
    if (bins, D) not in _EMBED:
        g = torch.Generator().manual_seed(1000 * bins + D)
        e = torch.randn(bins, D, generator=g) * 0.6
        e[1] = torch.where(torch.arange(D) % 2 == 0, 0.0, -0.0)
        e[2] = -30000.0
        _EMBED[(bins, D)] = (e, e.cuda())
    return _EMBED[(bins, D)]


def serial_scan(pval, pidx, bins):
    """vq_finalize's rule, part by part: the first part that reaches the maximum wins; an index outside [0, bins) gives 0."""
    codes = np.zeros(pval.shape[0], dtype=np.int64)
    for m in range(pval.shape[0]):
        best, bi = -math.inf, NO_INDEX
        for q in range(pval.shape[1]):
            if pval[m, q] > best:
                best, bi = pval[m, q], int(pidx[m, q])
        codes[m] = bi if 0 <= bi < bins else 0
    return codes


def build(rows, D, nparts, bins, seed):
    """Candidates and rows with the designed cases cycled over the rows: (what, row) pairs name them."""
    g = torch.Generator().manual_seed(seed)
    e, _ed = embed_of(bins, D)
    x = torch.randn(rows, D, generator=g) * 0.8
    pval = -torch.rand(rows, nparts, generator=g) * 10.0 - 1.0               # distances: negative, distinct with probability 1
    pidx = torch.randint(0, bins, (rows, nparts), generator=g, dtype=torch.int32)
    designed = []
    for m in range(rows):
        kind = m % 10
        if kind == 1 and nparts >= 2:            # equal maxima in two lanes (parts a < b): a wins
            a, b = sorted(torch.randperm(nparts, generator=g)[:2].tolist())
            pval[m, a] = pval[m, b] = -0.25
            pidx[m, a], pidx[m, b] = 3 % bins, 0
            designed.append(("tie across lanes", m))
        elif kind == 2 and nparts > 64:          # equal maxima in two parts of one lane's stride (q and q + 64): q wins
            q = int(torch.randint(0, nparts - 64, (1,), generator=g))
            pval[m, q] = pval[m, q + 64] = -0.125
            pidx[m, q], pidx[m, q + 64] = 1, 3 % bins
            designed.append(("tie inside a lane", m))
        elif kind == 3:                          # a row of NaN distances: every part reads (-inf, 0x7fffffff) -> code 0, r NaN
            pval[m] = -math.inf
            pidx[m] = NO_INDEX
            x[m, ::3] = math.nan
            designed.append(("nan row", m))
        elif kind == 4:                          # an empty last slab beside ordinary ones
            pval[m, nparts - 1] = -math.inf
            pidx[m, nparts - 1] = NO_INDEX
            designed.append(("empty slab", m))
        elif kind == 5:                          # x == embed[code]: every element +0
            c = int(torch.randint(0, bins, (1,), generator=g))
            q = int(torch.randint(0, nparts, (1,), generator=g))
            pval[m, q], pidx[m, q] = 0.0, c
            x[m] = e[c]
            designed.append(("exact", m))
        elif kind == 6:                          # zeros of both signs against row 1's
            q = int(torch.randint(0, nparts, (1,), generator=g))
            pval[m, q], pidx[m, q] = 0.0, 1
            x[m] = torch.where(torch.arange(D) % 4 < 2, -0.0, 0.0)
            designed.append(("signed zeros", m))
        elif kind == 7:                          # the maximum names an index outside the codebook: code 0
            q = int(torch.randint(0, nparts, (1,), generator=g))
            pval[m, q], pidx[m, q] = 0.5, bins + 5
            designed.append(("index outside", m))
        elif kind == 8 and nparts >= 2:          # a NaN candidate is never taken
            pval[m, nparts // 2] = math.nan
            designed.append(("nan candidate", m))
    return x, pval, pidx, designed


def run(x, pval, pidx, bins, s32, in_place=False):
    """One probe call -> (codes, r words, r_s32 words or None, xx words, status, form) and the bits the split and row_sumsq
    probes give on the returned r."""
    from wavtokenizer_amd import _capi
    rows, D = x.shape
    nparts = pval.shape[1]
    _e, ed = embed_of(bins, D)
    xd, pv, pi = x.contiguous().cuda(), pval.contiguous().cuda(), pidx.contiguous().cuda()
    co = Out(2 * rows, fill=-1431655766)
    ro, xo = Out(rows * D), Out(rows)
    so = Out(rows * D) if s32 else None
    if in_place:
        ro.buf[GUARD:GUARD + rows * D] = xd.view(torch.int32).reshape(-1)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _capi.WtVqResidualDesc()
    d.size = ctypes.sizeof(d)
    d.D, d.bins, d.nparts, d.rows = D, bins, nparts, rows
    d.pval, d.pidx, d.x, d.embed = pv.data_ptr(), pi.data_ptr(), ro.ptr if in_place else xd.data_ptr(), ed.data_ptr()
    d.codes, d.r, d.xx, d.status = co.ptr, ro.ptr, xo.ptr, status.data_ptr()
    if s32:
        d.r_s32 = so.ptr
    f = _capi.WtVqResidualForm()
    rc = _capi.lib.wt_vq_residual_probe(ctypes.byref(d), ctypes.byref(f), None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    # what the plans' own launchers make of the stored r
    sp = Out(rows * D)
    sd = _capi.WtSplitDesc()
    sd.size = ctypes.sizeof(sd)
    sd.op, sd.n, sd.x, sd.out = _capi.WT_SPLIT, rows * D, ro.ptr, sp.ptr
    assert _capi.lib.wt_split_probe(ctypes.byref(sd), None) == 0, _capi.lib.wt_last_error().decode()
    sq = Out(rows)
    od = _capi.WtOpDesc()
    od.size = ctypes.sizeof(od)
    od.op, od.n, od.C, od.x, od.y = _capi.WT_OP_ROW_SUMSQ, rows, D, ro.ptr, sq.ptr
    assert _capi.lib.wt_op_probe(ctypes.byref(od), None, None) == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    assert (f.grid, f.block, f.out_s32) == ((rows + 3) // 4, 256, 1 if s32 else 0)
    return (co.host().view(torch.int64).numpy(), ro.host().numpy(), so.host().numpy() if s32 else None, xo.host().numpy(),
            int(status[0]), sp.host().numpy(), sq.host().numpy())


def check(x, pval, pidx, bins, s32, what, want_status=0, in_place=False):
    e, _ed = embed_of(bins, x.shape[1])
    codes, r, rs, xx, status, split_ref, sumsq_ref = run(x, pval, pidx, bins, s32, in_place)
    want = serial_scan(pval.numpy(), pidx.numpy(), bins)
    assert np.array_equal(codes, want), f"{what}: codes differ at rows {np.nonzero(codes != want)[0][:6].tolist()}"
    want_r = (x.numpy().astype(np.float32) - e.numpy()[want]).astype(np.float32)
    got_r = r.view(np.float32).reshape(want_r.shape)
    nan = np.isnan(want_r)
    assert np.array_equal(np.isnan(got_r), nan), f"{what}: NaN rows must propagate NaN and nothing else may be NaN"
    same = (got_r.view(np.int32) == want_r.view(np.int32)) | nan             # (a NaN's payload is not a value)
    assert same.all(), f"{what}: {int((~same).sum())} words of r differ from float32(x) - embed[code], e.g. {np.argwhere(~same)[:3].tolist()}"
    if s32:
        assert np.array_equal(rs, split_ref), f"{what}: {int((rs != split_ref).sum())} words of r_s32 differ from split_s32 of the stored r"
    assert np.array_equal(xx, sumsq_ref), f"{what}: {int((xx != sumsq_ref).sum())} words of xx differ from row_sumsq of the stored r"
    assert status == want_status, f"{what}: status {status}, expected {want_status}"
    return codes, got_r


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("nparts", NPARTS)
def test_every_word_against_the_definition(nparts, D):
    n_designed = {}
    for bins in BINS:
        for rows in ROWS:
            x, pval, pidx, designed = build(rows, D, nparts, bins, seed=rows * 131 + nparts * 7 + D + bins)
            for s32 in (False, True):
                check(x, pval, pidx, bins, s32, f"rows {rows} D {D} nparts {nparts} bins {bins} s32 {s32}")
            for name, _m in designed:
                n_designed[name] = n_designed.get(name, 0) + 1
    must = {"nan row", "empty slab", "exact", "signed zeros", "index outside"} | ({"tie across lanes", "nan candidate"} if nparts >= 2 else set()) \
        | ({"tie inside a lane"} if nparts > 64 else set())
    assert must <= set(n_designed), (must - set(n_designed), n_designed)


def test_designed_rows_give_what_they_were_built_for():
    """The designed cases by their own expectations (not through the serial scan alone)."""
    D, nparts, bins, rows = 512, 172, 100, 65
    x, pval, pidx, designed = build(rows, D, nparts, bins, seed=5)
    codes, r = check(x, pval, pidx, bins, True, "designed")
    e, _ed = embed_of(bins, D)
    for name, m in designed:
        if name == "tie across lanes":
            assert codes[m] == 3
        elif name == "tie inside a lane":
            assert codes[m] == 1
        elif name in ("nan row", "index outside"):
            assert codes[m] == 0
        elif name == "exact":
            assert np.array_equal(r[m].view(np.int32), np.zeros(D, dtype=np.int32)), "x == embed[code] gives +0 in every element"
        elif name == "signed zeros":
            # -0 - +0 = -0, -0 - -0 = +0, +0 - +0 = +0, +0 - -0 = +0 (round to nearest)
            want = np.where((np.arange(D) % 4 < 2) & (np.arange(D) % 2 == 0), np.int32(-2 ** 31), np.int32(0))
            assert codes[m] == 1 and np.array_equal(r[m].view(np.int32), want)
    assert {n for n, _m in designed} >= {"tie across lanes", "tie inside a lane", "nan row", "exact", "signed zeros", "index outside"}


def test_in_place_residual_is_the_same_words():
    """The plans update the residual in place from round 1 on: r == x as one array."""
    x, pval, pidx, _designed = build(65, 512, 44, 4096, seed=11)
    a, ra = check(x, pval, pidx, 4096, True, "separate")
    b, rb = check(x, pval, pidx, 4096, True, "in place", in_place=True)
    assert np.array_equal(a, b) and np.array_equal(ra.view(np.int32), rb.view(np.int32))


def test_range_bit_when_the_residual_leaves_the_f16_range():
    """A forced code makes |r| reach 65504 while |x| stays below it: the S32 conversion reports WT_STATUS_BIT_RANGE; without the S32
    output nothing is converted and nothing is reported.  A NaN row beside it sets no bit."""
    from wavtokenizer_amd import _capi
    D, bins, nparts, rows = 512, 100, 7, 5
    x, pval, pidx, _designed = build(rows, D, nparts, bins, seed=3)          # row 3 is the NaN row
    assert bool(torch.isnan(x[3]).any())
    check(x, pval, pidx, bins, True, "nan row alone", want_status=0)
    x[0] = 0.5
    x[0, 17] = 40000.0
    pval[0, 2], pidx[0, 2] = 1.0, 2              # embed[2] = -30000: r = 70000
    assert float(x[torch.isfinite(x)].abs().max()) < 65504.0
    _codes, r = check(x, pval, pidx, bins, True, "overflow", want_status=_capi.WT_STATUS_BIT_RANGE)
    assert r[0, 17] == 70000.0
    check(x, pval, pidx, bins, False, "overflow, no S32 output", want_status=0)


def test_refused_descriptors_launch_nothing():
    from wavtokenizer_amd import _capi
    x, pval, pidx, _designed = build(4, 512, 2, 4, seed=1)
    _e, ed = embed_of(4, 512)
    xd, pv, pi = x.cuda(), pval.cuda(), pidx.cuda()
    co, ro, xo = Out(8, fill=-1431655766), Out(4 * 512), Out(4)

    def rc(**kw):
        d = _capi.WtVqResidualDesc()
        d.size = ctypes.sizeof(d)
        d.D, d.bins, d.nparts, d.rows = 512, 4, 2, 4
        d.pval, d.pidx, d.x, d.embed = pv.data_ptr(), pi.data_ptr(), xd.data_ptr(), ed.data_ptr()
        d.codes, d.r, d.xx = co.ptr, ro.ptr, xo.ptr
        for k, v in kw.items():
            setattr(d, k, v)
        return _capi.lib.wt_vq_residual_probe(ctypes.byref(d), None, None)

    for kw in (dict(D=384), dict(D=500), dict(x=None), dict(r=None), dict(codes=None), dict(nparts=0), dict(size=ctypes.sizeof(_capi.WtVqResidualDesc) - 8)):
        assert rc(**kw) == _capi.WT_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert bool((co.host() == -1431655766).all()) and bool((ro.host() == NAN_BITS).all()) and bool((xo.host() == NAN_BITS).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((ro.host() == NAN_BITS).all())
