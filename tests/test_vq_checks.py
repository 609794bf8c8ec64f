"""CPU-only half of tests/test_vq_ops.py: the bound and the checks of tests/vq_ref.py are honest (an fp32 evaluation in two
summation orders and a simulated split-f16 evaluation stay inside them on every element, with row_sumsq's |e|^2 table and,
handed to the reference as the operand it is, with the models' host-summed one) and sharp (each slip the argmax epilogue or vq_finalize could make puts at least one value, index, code or
feature word outside them), at shapes the GPU file uses; and the input builders keep their promises.  The evaluator here is
written on the launch geometry (slabs, parts, finalize lanes) independently of vq_ref's checks."""
import math

import pytest
import torch

from tests import vq_ref as V

SHAPES = [(4096, 512), (4100, 256), (100, 256), (16384, 512)]       # (bins, D)
ROWS = 96


# ------------------------------------------------------------------------------------------------ the evaluator
def _split(v, keep_lo=True):
    """The operands of gemm16s.hip as wt_vq_nearest prepares them: scaled per tensor by the power of two that brings the maximum
    into [1, 2), then hi = f16(v), lo = f16((v - hi) 2048)."""
    v = v.float()
    fin = v[torch.isfinite(v)].abs()
    amax = float(fin.max()) if fin.numel() else 0.0
    sc = 2.0 ** -math.floor(math.log2(amax)) if amax > 0 else 1.0
    vs = v * sc
    hi = vs.half().float()
    lo = ((vs - hi) * 2048.0).half().float()
    return hi, (lo if keep_lo else torch.zeros_like(lo)), sc


def _dot(x, e, mode):
    """x [rows][D] . e [bins][D] -> fp32 [rows][bins] in the arithmetic `mode` names."""
    if mode == "f32":                    # torch's blocked fp32 product
        return x.float() @ e.float().t()
    if mode == "f32rev":                 # one strictly serial fp32 chain, K descending
        x, e = x.float(), e.float()
        acc = torch.zeros(x.shape[0], e.shape[0], dtype=torch.float32)
        for k in range(x.shape[1] - 1, -1, -1):
            acc = acc + x[:, k:k + 1] * e[:, k]
        return acc
    if mode in ("s16", "s16_nolo_x", "s16_nolo_e"):      # hi + lo 2^-11 operands, lo.lo dropped, fp32 accumulation
        xh, xl, sx = _split(x, mode != "s16_nolo_x")
        eh, el, se = _split(e, mode != "s16_nolo_e")
        return ((xh @ eh.t()) + ((xl @ eh.t()) + (xh @ el.t())) * (1.0 / 2048.0)) * (1.0 / (sx * se))
    raise ValueError(mode)


def _sumsq(v):
    """row_sumsq_kernel: lane l holds channels 4 l .. 4 l + 3 of every 256-channel pass; (a + b) + (c + d) per pass, then the wave sum."""
    v = v.float()
    q = (v * v).reshape(v.shape[0], -1, 64, 4)                       # [rows][pass][lane][4]
    lane = torch.zeros(v.shape[0], 64, dtype=torch.float32)
    for p in range(q.shape[1]):
        lane = lane + ((q[:, p, :, 0] + q[:, p, :, 1]) + (q[:, p, :, 2] + q[:, p, :, 3]))
    n = 64
    while n > 1:
        lane = lane[:, :n // 2] + lane[:, n // 2:n]
        n //= 2
    return lane[:, 0]


def evaluate(case, mode, slip=None, ee_host=False, L=None):
    """(pval, pidx, codes, feat) of the kernels' arithmetic on the CPU: fp32 distances, the first strict maximum of every slab,
    vq_finalize's eight lanes over the parts and the transposed copy.  slip: one deliberate mistake."""
    x, e, kernel = case.x, case.embed, case.kernel
    bn, wn, nparts = V.geometry(kernel, case.bins)
    rows, bins = x.shape[0], e.shape[0]
    xx = _sumsq(x)
    ee = V.host_serial_ee(e) if ee_host else _sumsq(e)
    if slip == "ee_neighbour":
        ee = torch.roll(ee, -1)
    if slip == "ee_zero_tail":           # the last 4-column run reads no table
        ee = ee.clone()
        ee[4 * ((bins - 1) // 4):] = 0
    if slip == "no_xx":
        xx = torch.zeros_like(xx)
    dot = _dot(x, e, mode)
    d = -((xx[:, None] - 2.0 * dot) + ee[None, :])
    nan = torch.isnan(d)
    d = torch.where(nan, torch.full_like(d, -math.inf), d)
    pad = torch.full((rows, nparts * wn), -math.inf)
    pad[:, :bins] = d
    live = torch.zeros(rows, nparts * wn, dtype=torch.bool)
    live[:, :bins] = ~nan
    sl, lv = pad.reshape(rows, nparts, wn), live.reshape(rows, nparts, wn)
    pval = sl.max(-1).values
    hit = (sl == pval[..., None]) & lv
    if kernel == 0:                      # a strict '>' from -inf never takes a -inf
        hit = hit & (sl > -math.inf)
    first = V._first(hit)
    last = wn - 1 - V._first(hit.flip(-1))
    loc = last if slip == "ge_slab" else first
    start = torch.arange(nparts) * wn
    base = start % bn if slip == "no_tile_offset" else start
    pidx = torch.where(hit.any(-1), loc + base[None, :], torch.full_like(loc, V.NO_INDEX))
    # vq_finalize: lane `sub` scans parts sub, sub + 8, .. ascending with a strict '>', then the lanes merge on (value, part)
    best = torch.full((rows,), -math.inf)
    bi = torch.full((rows,), V.NO_INDEX)
    order = range(nparts)
    if slip == "finalize_high_first":
        order = sorted(range(nparts), key=lambda q: (-(q % 8), q))   # lanes merged highest lane first: on ties the highest lane's part
    for q in order:
        take = (pval[:, q] >= best) if slip == "ge_finalize" else (pval[:, q] > best)
        best = torch.where(take, pval[:, q], best)
        bi = torch.where(take, pidx[:, q], bi)
    codes = torch.where((bi < 0) | (bi >= bins), torch.zeros_like(bi), bi)
    feat = None
    if L is not None:
        B = rows // L
        src = codes.reshape(B, L).clone()
        if slip == "feat_tail_prev_tile" and L > 32 and L % 32:
            t0 = L - L % 32
            src[:, t0:] = src[:, t0 - 32:t0 - 32 + L % 32]
        feat = e[src].transpose(1, 2).contiguous()
    return pval, pidx, codes, feat


_CASES = {}


def case_of(bins, D, kernel, rows=ROWS, special=True):
    key = (bins, D, kernel, rows, special)
    if key not in _CASES:
        _CASES[key] = V.Case(bins, D, rows, kernel, seed=bins + D + kernel, special=special)
    return _CASES[key]


def run_checks(case, out, ee=None):
    pval, pidx, codes, feat = out
    ref = case.ref(ee)
    frac, _s, _n = V.check_parts(pval, pidx, V.Form.of(case.kernel, case.bins), None, None, ref=ref)
    V.check_codes(codes, None, None, ref=ref)
    case.check_designed(codes, near=ee is None)
    if feat is not None:
        V.check_feat(feat, codes, case.embed)
    return frac


# ------------------------------------------------------------------------------------------------ honest evaluations pass
@pytest.mark.parametrize("bins,D", SHAPES)
@pytest.mark.parametrize("mode,kernel", [("f32", 1), ("f32rev", 1), ("s16", 0)])
def test_honest_evaluations_are_inside_the_bounds(bins, D, mode, kernel):
    c = case_of(bins, D, kernel)
    L = 32
    frac = run_checks(c, evaluate(c, mode, L=L))
    # the models' host-summed table is an operand: the reference is handed the same one
    ee = V.host_serial_ee(c.embed)
    frac_h = run_checks(c, evaluate(c, mode, ee_host=True, L=L), ee=ee)
    print(f"bins {bins} D {D} {mode}: worst value error {frac:.3g} of the bound ({frac_h:.3g} with the host-summed table)")


@pytest.mark.parametrize("bins,D", SHAPES)
def test_host_summed_table_is_an_operand(bins, D):
    """weights.cpp sums |e|^2 in one serial fp32 chain of D terms: within D / 2 roundings of float64, which is more than row_sumsq's 12.
    On the all-zero row (distance -ee[n], nothing else to hide behind) the evaluation that used it leaves the bound taken against the
    float64 |e|^2 at the larger codebooks, which is why the checks are handed the table whenever the kernels were."""
    c = case_of(bins, D, 1)
    ee = V.host_serial_ee(c.embed)
    e64 = (c.embed.double() ** 2).sum(1)
    worst = float(((ee.double() - e64).abs() / e64).max())
    print(f"bins {bins} D {D}: host-summed table within {worst / 2.0 ** -23:.3g} x 2^-23 of float64")
    assert worst <= D / 2 * 2.0 ** -24
    if worst > V.C * V.ULP:
        with pytest.raises(AssertionError, match="values outside the bound"):
            run_checks(c, evaluate(c, "f32", ee_host=True))


@pytest.mark.parametrize("bins,D,kernel", [(4, 256, 0), (4, 256, 1), (96, 256, 0), (192, 512, 0), (384, 768, 1), (100, 768, 1), (99, 256, 1)])
def test_honest_small_codebooks(bins, D, kernel):
    c = case_of(bins, D, kernel, rows=40)
    run_checks(c, evaluate(c, "s16" if kernel == 0 else "f32", L=20))


# ------------------------------------------------------------------------------------------------ slips fail
SLIPS = ["ee_neighbour", "ee_zero_tail", "ge_slab", "ge_finalize", "no_tile_offset", "finalize_high_first", "feat_tail_prev_tile"]


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("slip", SLIPS)
def test_slips_are_outside_the_bounds(slip, kernel):
    c = case_of(4096, 512, kernel)
    with pytest.raises(AssertionError):
        run_checks(c, evaluate(c, "s16" if kernel == 0 else "f32", slip=slip, L=48))


@pytest.mark.parametrize("bins,D", SHAPES)
@pytest.mark.parametrize("slip", ["s16_nolo_x", "s16_nolo_e"])
def test_a_dropped_lo_half_is_outside_the_bounds(slip, bins, D):
    """Either half shows in the values (check_parts) at every shape.  In the codes, a dropped lo half of the codebook flips designed
    near-tie rows at every shape.  A dropped lo half of x does not have to: on these rows x is the mean of two codebook rows, the
    dropped half moves d[a] - d[b] by about 3e-3 (rms), and the rows sit 2.05 bounds = 8e-3 apart because gemm_ref.TOL grants
    gemm16s three times its worst case; a row closer than that is a row a correct kernel may flip too."""
    c = case_of(bins, D, 0)
    out = evaluate(c, slip)
    with pytest.raises(AssertionError):
        V.check_parts(out[0], out[1], V.Form.of(0, bins), None, None, ref=c.ref())
    flipped = [r for r in c.near_rows if int(out[2][r]) != c.want[r]]
    print(f"{slip} bins {bins}: {len(flipped)} of {len(c.near_rows)} near-tie rows flipped")
    if slip == "s16_nolo_e":
        assert flipped, "no designed row noticed the dropped half"
        with pytest.raises(AssertionError):
            c.check_designed(out[2])


@pytest.mark.parametrize("kernel", [0, 1])
def test_omitted_xx_shows_in_the_values_only(kernel):
    """xx is the same for every column of a row: leaving it out moves no argmax, so only check_parts' value condition sees it."""
    c = case_of(4096, 512, kernel, special=False)
    pval, pidx, codes, _f = evaluate(c, "s16" if kernel == 0 else "f32", slip="no_xx")
    V.check_codes(codes, None, None, ref=c.ref())
    with pytest.raises(AssertionError, match="values outside the bound"):
        V.check_parts(pval, pidx, V.Form.of(kernel, 4096), None, None, ref=c.ref())


# ------------------------------------------------------------------------------------------------ the builders keep their promises
@pytest.mark.parametrize("bins,D", SHAPES)
@pytest.mark.parametrize("kernel", [0, 1])
def test_builders_keep_their_promises(bins, D, kernel):
    c = case_of(bins, D, kernel)
    ref = c.ref()
    assert len(c.near_rows) >= 8 and len(c.sets) >= (10 if bins >= 4096 else 8), (len(c.near_rows), len(c.sets))
    # every designed near-tie row: the winner's float64 margin over every other column exceeds 2 bound, and is no wider than M_TIE asks
    for r in c.near_rows:
        a = c.want[r]
        gap = ref.d[r, a] - ref.d[r]
        room = ref.b[r, a] + ref.b[r]
        gap[a], room[a] = math.inf, 1.0
        assert bool((gap > room).all()), (r, a, float((gap / room).min()))
        assert float((gap / room).min()) < (V.M_TIE + 0.1) / 2, (r, a, float((gap / room).min()))
    # the designed case as a whole (duplicates included), then random rows: those allowed more than one answer are at most 1 %
    loose, n = V.undecidable(ref)
    assert 100 * loose <= n, (loose, n)
    nudged = V.Ref(c.x, c.embed, kernel)                 # a float64 product that does not give bit-identical columns equal distances
    nudged.d = ref.d.clone()
    for s in c.sets:
        nudged.d[:, s[-1]] += 1e-13
    assert V.undecidable(nudged) == (loose, n)
    rnd = V.Case(bins, D, 400, kernel, seed=7 + bins, special=False, designed=False)
    loose, n = V.undecidable(V.Ref(rnd.x, rnd.embed, kernel))
    print(f"bins {bins} D {D} kernel {kernel}: {loose} of {n} random rows within 2 bound of a tie")
    assert 100 * loose <= n


def test_tie_sets_follow_the_geometry():
    for kernel in (0, 1):
        for bins in (4, 96, 100, 192, 384, 4096, 4100, 16384):
            bn, wn, nparts = V.geometry(kernel, bins)
            sets, used = V.tie_sets(bins, bn, wn)
            assert sets and all(s[-1] < bins for s in sets) and sum(len(s) for s in sets) == len(used)
            if bins >= 4096:
                spans = {(s[0] // wn != s[-1] // wn, s[0] // bn != s[-1] // bn, (s[-1] // wn - s[0] // wn) % 8 == 0 and s[0] // wn != s[-1] // wn) for s in sets}
                assert (False, False, False) in spans and (True, False, False) in spans and (True, True, False) in spans and (True, True, True) in spans
                assert any(len(s) == 3 for s in sets) and (0, bins - 1) in sets


def test_model_create_refuses_a_codebook_the_vq_kernel_cannot_take():
    """vq_bins % 4 != 0: gemm16s.hip's argmax epilogue reads |e|^2 four columns at a time (check_gemm16s refuses such an N), so
    the model is refused before anything is uploaded (no GPU needed)."""
    import ctypes
    from wavtokenizer_amd import _capi, NAMED_ARCHS
    arch = NAMED_ARCHS["hop600"]
    for bins in (4098, 2, 0):
        wa = _capi.WtArch()
        wa.n_ratios = len(arch.ratios)
        for i, r in enumerate(arch.ratios):
            wa.ratios[i] = r
        wa.vq_bins, wa.num_quantizers, wa.input_channels = bins, arch.num_quantizers, arch.input_channels
        wa.dim, wa.intermediate_dim, wa.num_layers = arch.dim, arch.intermediate_dim, arch.num_layers
        wa.adanorm_num_embeddings, wa.n_fft, wa.hop_length = arch.adanorm_num_embeddings, arch.n_fft, arch.hop_length
        out = ctypes.c_void_p()
        t = (_capi.WtTensor * 1)()
        rc = _capi.lib.wt_model_create(ctypes.byref(wa), t, 0, 0, ctypes.byref(out))
        assert rc == _capi.WT_ERR_INVALID and b"vq_bins" in _capi.lib.wt_last_error() and not out.value
