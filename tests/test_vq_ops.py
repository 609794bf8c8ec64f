"""The vector quantiser's kernels alone, through wt_vq_probe (the encoder plan's own launchers: row_sumsq, the distance GEMM with
the argmax epilogue on gemm16s.hip (kernel 0) or gemm.hip (kernel 1), one vq_finalize), against the float64 reference and the
derived bound of tests/vq_ref.py.  Per case: (a) the launch form the probe reports is the one the case is sized for; (b) every
partial (value, index) candidate of every row against the slab it covers, every code and every feature word (vq_ref.check_parts,
check_codes, check_feat: no sampling, no element excluded); (c) the designed rows (exact duplicates across every merge level,
near ties in both orders, a zero row, a NaN row, an overflowing row) give the code they were built for; (d) the guard words
around the NaN / sentinel pre-filled outputs untouched and the status word clear.  Then the shipped encode plans' own VQ buffers
in place, plain and mixed-length.  The last test compares the forms the session reached with the ones the launchers can pick.
tests/test_vq_checks.py holds the CPU half: the bound passes honest evaluations and rejects the slips."""
import ctypes

import pytest
import torch

from tests import parity_log
from tests import vq_ref as V
from tests.util import synth_state_dict

pytestmark = pytest.mark.gpu

GUARD = 64                       # 32-bit words of sentinel before and after every output
SENT = -559038737                # 0xDEADBEEF
NAN_BITS = 0x7FC00000
HIT = set()                      # (kernel, wrapped, group_m, a part of the last column tile: "empty" / "partial" / "full") reached in this session
WORST = {}                       # kernel -> worst |pval - slab maximum| / bound
BINS = [4, 96, 100, 192, 384, 4096, 4100, 16384]
ROWS = [1, 31, 32, 33, 127, 128, 129, 1000]
CLIPS = [(1, 1), (3, 33), (2, 64), (5, 31), (1, 1000)]


class Out:
    """A device output of n 32-bit words between two guard runs, pre-filled (NaN bits: every logical element must be written)."""

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


def ncu():
    from wavtokenizer_amd import _capi
    cu = ctypes.c_int32()
    assert _capi.lib.wt_device_info(torch.cuda.current_device(), ctypes.byref(cu), None, None) == 0
    return cu.value


def desc(kernel, B, L, D, bins):
    from wavtokenizer_amd import _capi
    d = _capi.WtVqDesc()
    d.size = ctypes.sizeof(d)
    d.kernel, d.B, d.L, d.D, d.bins = kernel, B, L, D, bins
    return d


def run_vq(x, embed, kernel, B, L, ee=None, feat=True):
    """One probe call -> (form, pval [rows][nparts] fp32, pidx int32, codes [rows] int64, feat [B][D][L] fp32 or None)."""
    from wavtokenizer_amd import _capi
    rows, D = x.shape
    bins = embed.shape[0]
    assert rows == B * L
    nparts = V.geometry(kernel, bins)[2]
    d = desc(kernel, B, L, D, bins)
    keep = [x.float().contiguous().cuda(), embed.float().contiguous().cuda()]
    d.x, d.embed = keep[0].data_ptr(), keep[1].data_ptr()
    if ee is not None:
        keep.append(ee.float().contiguous().cuda())
        d.ee = keep[2].data_ptr()
    pv, pi = Out(rows * nparts), Out(rows * nparts)
    co = Out(2 * rows, fill=-1431655766)                # 0xAAAAAAAA: an int64 far outside any codebook
    ft = Out(B * D * L) if feat else None
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    d.pval, d.pidx, d.codes, d.status = pv.ptr, pi.ptr, co.ptr, status.data_ptr()
    if feat:
        d.feat = ft.ptr
    ws = torch.empty(_capi.lib.wt_vq_workspace_bytes(rows, D, bins) + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) // 256 * 256
    f = _capi.WtVqForm()
    rc = _capi.lib.wt_vq_probe(ctypes.byref(d), ctypes.byref(f), wp, None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    assert int(status[0]) == 0, f"status {int(status[0])} on an in-range problem"
    assert f.nparts == nparts and f.fin_grid_x == -(-L // 32) and f.fin_grid_y == B
    return (f, pv.host().view(torch.float32).reshape(rows, nparts), pi.host().reshape(rows, nparts), co.host().view(torch.int64),
            ft.host().view(torch.float32).reshape(B, D, L) if feat else None)


def check_form(f, kernel, rows, bins):
    """The tile form and grid launch16s_tiled / launch_tiled pick for the argmax epilogue, and the tile order of launch_gemm16s /
    launch_gemm; records which forms the session reached."""
    bn, wn, nparts = V.geometry(kernel, bins)
    tiles_n = -(-bins // bn)
    ntiles = -(-rows // 128) * tiles_n
    assert (f.BM, f.BN, f.waves_m, f.waves_n) == ((128, 192, 4, 2) if kernel == 0 else (128, 128, 2, 2)), (f.BM, f.BN, f.waves_m, f.waves_n)
    assert f.ntiles == ntiles and f.nparts == 2 * tiles_n
    if kernel == 0:
        slots = ncu() & ~7                               # 4 x 2 waves: one workgroup per CU, a multiple of 8
        if slots < 8 or ntiles <= slots:
            assert f.grid == ntiles, (f.grid, ntiles)
        else:
            rounds = -(-ntiles // slots)
            assert f.grid == min(slots, (-(-ntiles // rounds) + 7) & ~7), (f.grid, ntiles, slots)
        gm, gn = (5, 6) if tiles_n >= 12 and tiles_n % 6 == 0 else ((8, 0) if tiles_n > 8 else (1, 0))
    else:
        assert f.grid == ntiles                          # gemm.hip has no persistent form
        gm, gn = (8 if -(-bins // (32 if bins <= 32 else 64 if bins <= 64 else 96)) > 8 else 1), 0
    assert (f.group_m, f.group_n) == (gm, gn), (f.group_m, f.group_n, gm, gn)
    for q in (nparts - 2, nparts - 1):                   # the two parts of the last column tile
        cols = min(max(bins - q * wn, 0), wn)
        HIT.add((kernel, f.grid < f.ntiles, f.group_m, "empty" if cols == 0 else "full" if cols == wn else "partial"))


def check_case(c, B, L, ee=None, what=""):
    f, pval, pidx, codes, feat = run_vq(c.x, c.embed, c.kernel, B, L, ee=ee)
    check_form(f, c.kernel, c.rows, c.bins)
    ref = c.ref(ee)
    frac, strict, n = V.check_parts(pval, pidx, f, None, None, ref=ref, what=f"{what} parts")
    srows, nrows = V.check_codes(codes, None, None, ref=ref, what=f"{what} codes")
    V.check_feat(feat, codes, c.embed, what=f"{what} feat")
    c.check_designed(codes, what=f"{what} designed rows", near=ee is None)
    print(f"{what}: worst value error {frac:.3g} of the bound; {strict} of {n} candidates and {srows} of {nrows} codes decidable exactly")
    WORST[c.kernel] = max(WORST.get(c.kernel, 0.0), frac)
    return f


_CASES = {}


def case_of(bins, D, rows, kernel, **kw):
    key = (bins, D, rows, kernel, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES.clear()                                   # (one at a time: a 16384-column reference is 100 MB)
        _CASES[key] = V.Case(bins, D, rows, kernel, seed=bins + D + rows + kernel, **kw)
    return _CASES[key]


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("kernel", [0, 1])
def test_codebook_sizes(kernel, bins):
    """The smallest legal codebook, exactly one wave slab of gemm16s, a 4-column second slab, one and two full tiles, the shipped
    size (its last part empty on gemm16s), a 68-column last tile, the reference's default (group_m = 8, 86 column tiles); 129
    rows = two row tiles, the second with one row.  The two shipped sizes also with the models' host-summed |e|^2 table."""
    c = case_of(bins, 512, 129, kernel)
    check_case(c, 3, 43, what=f"kernel {kernel} bins {bins}")
    if bins in (4096, 16384):
        check_case(c, 3, 43, ee=V.host_serial_ee(c.embed), what=f"kernel {kernel} bins {bins} host table")
    loose, n = V.undecidable(c.ref())
    assert 100 * loose <= n, f"{loose} of {n} rows are allowed more than one answer"


@pytest.mark.parametrize("bins", [98, 197, 4099])
def test_codebook_sizes_off_four_fp32(bins):
    """gemm.hip's argmax epilogue reads |e|^2 one column at a time: any bins >= 1 is supported on kernel 1, and tested like the rest
    (the split-f16 kernel refuses such a codebook: test_refusals)."""
    check_case(case_of(bins, 256, 70, 1), 2, 35, what=f"kernel 1 bins {bins}")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kernel", [0, 1])
def test_row_counts(kernel, rows):
    """Around one row tile (128) and one finalize tile (32), one row, several row tiles."""
    check_case(case_of(384, 256, rows, kernel), 1, rows, what=f"kernel {kernel} rows {rows}")


@pytest.mark.parametrize("D", [256, 768])
@pytest.mark.parametrize("kernel", [0, 1])
def test_codebook_widths(kernel, D):
    """One and three 256-channel passes of vq_finalize and row_sumsq (512: every other case)."""
    check_case(case_of(4100, D, 66, kernel), 2, 33, what=f"kernel {kernel} D {D}")


@pytest.mark.parametrize("B,L", CLIPS)
@pytest.mark.parametrize("kernel", [0, 1])
def test_clip_forms(kernel, B, L):
    """vq_finalize with features over B clips of L frames: one frame, a tail tile of one frame, whole tiles, a tail of 31, rows
    that cross clip boundaries inside a 128-row GEMM tile."""
    check_case(case_of(192, 768, B * L, kernel), B, L, what=f"kernel {kernel} clips {B} x {L}")


@pytest.mark.parametrize("bins", [4096, 16384])
@pytest.mark.parametrize("kernel", [0, 1])
def test_more_tiles_than_workgroups(kernel, bins):
    """gemm16s (kernel 0): more output tiles than resident workgroups, so the persistent form walks tiles b, b + G, ... and the
    argmax epilogue runs at every tile seam, in groups of 8 row tiles (both sizes have more than 8 column tiles).  gemm.hip
    (kernel 1) has no persistent form: the same rows launch one workgroup per tile, which the form must say."""
    bn = V.geometry(0, bins)[0]
    rows = 128 * (ncu() // -(-bins // bn) + 1) + 1
    c = case_of(bins, 512, rows, kernel)
    f = check_case(c, 1, rows, what=f"kernel {kernel} bins {bins} rows {rows}")
    if kernel == 0:
        assert f.grid < f.ntiles and f.BN == 192 and (f.waves_m, f.waves_n) == (4, 2) and f.group_m == 8, (f.grid, f.ntiles, f.group_m)
        assert f.nparts == 2 * -(-bins // 192)
    else:
        assert f.grid == f.ntiles and f.nparts == 2 * -(-bins // 128)


def test_refusals():
    """Host only: each of these returns WT_ERR_INVALID with a message before any launch (the outputs keep their pre-fill)."""
    from wavtokenizer_amd import _capi
    x = torch.zeros(64, 512, device="cuda")
    e = torch.zeros(200, 512, device="cuda")
    ws = torch.empty(_capi.lib.wt_vq_workspace_bytes(64, 512, 200) + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) // 256 * 256
    for kernel, D, bins, word in ((0, 512, 198, "gemm16s"), (0, 512, 2, "gemm16s"), (0, 288, 200, "256"), (1, 288, 200, "256"), (1, 130, 200, "D % 4"),
                                  (2, 512, 200, "kernel"), (0, 512, 0, "bins")):
        d = desc(kernel, 2, 32, D, bins)
        pv, pi, co, ft = Out(64 * 4), Out(64 * 4), Out(128), Out(64 * 512)
        d.x, d.embed, d.pval, d.pidx, d.codes, d.feat = x.data_ptr(), e.data_ptr(), pv.ptr, pi.ptr, co.ptr, ft.ptr
        rc = _capi.lib.wt_vq_probe(ctypes.byref(d), None, wp, None)
        msg = _capi.lib.wt_last_error().decode()
        assert rc == _capi.WT_ERR_INVALID and word in msg, (kernel, D, bins, rc, msg)
        torch.cuda.synchronize()
        for o in (pv, pi, ft):
            assert bool((o.host() == NAN_BITS).all()), (kernel, D, bins, "an output was written")
    d = desc(0, 2, 32, 512, 200)
    d.size -= 8
    assert _capi.lib.wt_vq_probe(ctypes.byref(d), None, wp, None) == _capi.WT_ERR_INVALID


# ------------------------------------------------------------------------------------------------ the shipped plans' VQ, in place
@pytest.fixture(scope="module", params=["hop600", "hop320"])
def model(request):
    from wavtokenizer_amd import WavTokenizer, NAMED_ARCHS
    sd = synth_state_dict(request.param)
    m = WavTokenizer.from_arch(NAMED_ARCHS[request.param])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    embed = torch.from_numpy(sd["feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed"]).float()
    return request.param, m.eval().to("cuda"), embed


def _plan_buffer(plan, ws, name, must=True):
    """A named fp32 buffer of a plan's workspace after a run (None, with must = False, if the plan has none of that name)."""
    from wavtokenizer_amd import _capi
    off, n, fmt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
    rc = _capi.lib.wt_plan_buffer_info(plan, name.encode(), ctypes.byref(off), ctypes.byref(n), ctypes.byref(fmt))
    if rc != 0 and not must:
        return None
    assert rc == 0 and fmt.value == 0, (name, rc, fmt.value)
    return ws[off.value: off.value + 4 * n.value].view(torch.float32).cpu()


def _has_buffer(plan, name):
    from wavtokenizer_amd import _capi
    off, n, fmt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
    return _capi.lib.wt_plan_buffer_info(plan, name.encode(), ctypes.byref(off), ctypes.byref(n), ctypes.byref(fmt)) == 0


def _check_plan_vq(plan, ws, embed, B, Lpad, lengths, feats, codes, what):
    """check_parts / check_codes / check_feat on a plan's own VQ buffers after a run: the embedding that fed the VQ (the fp32 twin of
    the S32 tensor the distance GEMM read), vq.xx, vq.pval, vq.pidx; valid frames of every clip."""
    bins = embed.shape[0]
    last = max(k for k in range(40) if _has_buffer(plan, f"enc.{k}"))          # the final conv's output: fp32, with an S32 twin
    assert _has_buffer(plan, f"enc.{last}.s32")
    emb = _plan_buffer(plan, ws, f"enc.{last}").reshape(B * Lpad, 512)
    xx = _plan_buffer(plan, ws, "vq.xx").reshape(B * Lpad)
    pval = _plan_buffer(plan, ws, "vq.pval").reshape(B * Lpad, -1)
    pidx = _plan_buffer(plan, ws, "vq.pidx").view(torch.int32).reshape(B * Lpad, -1)
    nparts = pval.shape[1]
    assert nparts == V.geometry(0, bins)[2], "the shipped plan runs the distances on gemm16s.hip"
    rows = torch.cat([b * Lpad + torch.arange(lengths[b]) for b in range(B)])
    x = emb[rows]
    x64 = (x.double() ** 2).sum(1)
    assert bool(((xx[rows].double() - x64).abs() <= 12 * 2.0 ** -24 * x64).all()), f"{what}: vq.xx outside row_sumsq's 12 roundings"
    ee = V.host_serial_ee(embed)                          # weights.cpp's table, the operand the plan's GEMM reads
    ref = V.Ref(x, embed, 0, ee)
    frac, strict, n = V.check_parts(pval[rows], pidx[rows], V.Form.of(0, bins), None, None, ref=ref, what=f"{what} parts")
    got = torch.cat([codes[0, b, :lengths[b]] for b in range(B)]).cpu()
    srows, nrows = V.check_codes(got, None, None, ref=ref, what=f"{what} codes")
    for b in range(B):
        V.check_feat(feats[b:b + 1, :, :lengths[b]].cpu(), codes[0, b, :lengths[b]].cpu(), embed, what=f"{what} feat clip {b}")
    print(f"{what}: worst value error {frac:.3g} of the bound; {strict} of {n} candidates, {srows} of {nrows} codes decidable exactly")
    parity_log.record(f"vq_ops {what}", worst_of_bound=frac, decidable_codes=srows, rows=nrows)
    return frac


def test_shipped_plan_vq_in_place(model):
    """The default encode plan with its stage buffers kept: B = 3, 37 frames (no multiple of 32).  The VQ is judged on the
    embedding the plan itself produced, so upstream error plays no part and the arithmetic bound stands in for NEAR_TIE_MARGIN."""
    from wavtokenizer_amd import _capi, synth
    name, m, embed = model
    B, L = 3, 37
    T = m.arch.hop * L
    wav = torch.from_numpy(synth.make_clips(B, T, seed=321)).cuda()
    m.set_debug_keep_stages(True)
    try:
        feats, codes = m.encode_infer(wav, bandwidth_id=torch.tensor([0]))
        torch.cuda.synchronize()
        assert codes.shape == (1, B, L) and feats.shape == (B, 512, L)
        plan, ws = m._engine.plans[(_capi.WT_PLAN_ENCODE, B, T, m._plan_flags)]
        _check_plan_vq(plan, ws, embed, B, L, [L] * B, feats, codes, f"plan {name}")
    finally:
        m.set_debug_keep_stages(False)


def test_mixed_length_plan_vq_in_place(model):
    """The mixed-length twin (what encode_infer_many runs): each clip's valid frames the same way; past each clip's frames codes
    -1 and features 0 (mixed_pad).  The VQ's buffers are live until the plan's last step, so they are read without KEEP_STAGES."""
    from wavtokenizer_amd import _capi, synth
    from wavtokenizer_amd.mixed_length import group_clips
    name, m, embed = model
    hop = m.arch.hop
    lengths = [hop * 37, hop * 21 + 5, hop * 30 - 7]
    wavs = [torch.from_numpy(synth.make_clips(1, T, seed=500 + i)[0].copy()).cuda() for i, T in enumerate(lengths)]
    groups, solo = group_clips(lengths, hop)
    assert not solo and len(groups) == 1
    T_pad, idx = groups[0]
    dev = m._ensure_engine()
    m._engine.drop(lambda k: k[0] == _capi.WT_PLAN_ENCODE)
    res = m._run_encode_mixed([wavs[i] for i in idx], T_pad, dev)
    assert res is not None, "the encoder is off the mixed-length route"
    feats, codes = res
    torch.cuda.synchronize()
    keys = [k for k in m._engine.plans if k[0] == _capi.WT_PLAN_ENCODE and k[3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH]
    assert len(keys) == 1
    plan, ws = m._engine.plans[keys[0]]
    Lpad = codes.shape[2]
    frames = [-(-lengths[i] // hop) for i in idx]
    _check_plan_vq(plan, ws, embed, len(idx), Lpad, frames, feats, codes, f"mixed plan {name}")
    for b, Lb in enumerate(frames):
        assert bool((codes[0, b, Lb:] == -1).all()) and bool((feats[b, :, Lb:] == 0).all()), f"clip {b}: padding past its {Lb} frames"


def test_every_form_was_reached():
    """Runs last: plain and wrapped grids, group_m 1 and 8, an empty, a partial and a full last part, on each kernel that has the
    form; the worst fraction of the bound per kernel goes to the parity log (none above 1: the cases assert it)."""
    for kernel, w in sorted(WORST.items()):
        parity_log.record(f"vq_ops kernel {kernel} ({'gemm16s' if kernel == 0 else 'gemm'})", worst_of_bound=w)
    want = {(k, False, gm, part) for k in (0, 1) for gm in (1, 8) for part in ("empty", "partial", "full")} - {(0, False, 8, "full")}
    want |= {(0, True, 8, "empty"), (0, True, 8, "partial")}
    assert HIT >= want, want - HIT
    assert not [h for h in HIT if h[0] == 1 and h[1]], "gemm.hip has no persistent form"
