"""Float64 reference, per-element bound, checks and seeded input builders for the vector quantiser (tests/test_vq_ops.py on
the GPU, tests/test_vq_checks.py on the CPU): EuclideanCodebook.quantize (core_vq.py:175-183) as the encoder plan runs it,
row_sumsq -> distance GEMM with the per-slab argmax epilogue -> vq_finalize.  Everything here is built from the definition
and from the launch geometry the probe reports, never from a kernel output.  CPU only.

The bound.  A kernel computes d[m][n] = -((xx[m] - 2 dot[m][n]) + ee[n]) in fp32.  With u = 2^-24 (one rounding) and
T = xx + 2 sum_i |x_i e_i| + ee:
  * xx and ee come from row_sumsq: a product (1 rounding), two additions inside a lane's four values (2), one accumulation
    per 256-channel pass (D / 256 <= 3) and the six levels of the wave sum (6): at most 12 roundings on a sum of
    non-negative terms, 12 u xx and 12 u ee;
  * the dot product on the fp32 MFMA chain (kernel 1): products are exact in the accumulator, the accumulation over K costs at
    most (K / 32 + 5) u sum|x e| (the model tests/gemm_ref.py uses), 29 u sum|x e| at K = 768; 2 dot is exact;
  * the epilogue: two additions, u (xx + 2 sum|x e|) and u T.  The negation is exact.
  In units of 2^-23 = 2 u that is 7 (xx + ee) + 8.25 (2 sum|x e|), and since 2 sum|x e| <= xx + ee this is at most
  8 . 2^-23 . T: C = 8.  It is a worst case for row_sumsq and the epilogue and the project's model for the accumulation;
  nothing in it was read off a GPU.
  * kernel 0 (gemm16s.hip) multiplies split-f16 operands (hi + lo 2^-11, lo.lo dropped): gemm_ref.TOL on sum|x e| covers the
    split form and its accumulation, twice because the distance holds 2 dot; the f16 subnormal floor of the lo halves of the
    operands (scaled per tensor to a maximum in [1, 2) by the probe, unscaled in the plans) adds 2^-36 max(1, max|x|) per element of x
    and 2^-36 max(1, max|e|) per element of e.
A table `ee` handed to the probe (the models' host-summed one) is an operand, not a result: the reference then takes it as
it is.  tests/test_vq_checks.py shows separately how far such a table is from float64.

Rows that fp32 cannot order are defined by what the kernels document: a row that holds a NaN selects nothing (every part
(-inf, 0x7fffffff), code 0, vq_finalize_kernel); a finite row whose |x|^2 overflows fp32 has every distance -inf (kernel 1:
each part names its first column, code 0, as torch.max gives)."""
import math

import torch

from tests import gemm_ref as G

C = 8.0
ULP = 2.0 ** -23
FLT_MAX = 3.4028234663852886e38
NO_INDEX = 0x7FFFFFFF
M_TIE = 2.05         # margin of a designed near-tie row in units of (bound[a] + bound[b]) / 2: the strict criterion needs more than 2, and
                     # the margin is computed from the rounded x, so nothing else has to fit; the smallest such multiple is also the
                     # one at which a dropped lo half of the codebook flips designed rows (tests/test_vq_checks.py proves both sides)


def geometry(kernel, bins):
    """What launch16s_tiled / launch_tiled pick for the argmax epilogue: (BN, WN, nparts)."""
    bn, wn = (192, 96) if kernel == 0 else (128, 64)
    return bn, wn, 2 * -(-bins // bn)


class Form:
    """The fields of wt_vq_form the checks read (the CPU tests build one from geometry())."""

    def __init__(self, BN, waves_n, nparts):
        self.BN, self.waves_n, self.nparts = BN, waves_n, nparts

    @classmethod
    def of(cls, kernel, bins):
        bn, _wn, nparts = geometry(kernel, bins)
        return cls(bn, 2, nparts)


def distances(x, embed, ee=None):
    """float64 -(|x|^2 - 2 x.e + |e|^2), [rows][bins]; ee: a table to use in place of |e|^2."""
    x, e = x.double(), embed.double()
    ee = (e * e).sum(1) if ee is None else ee.double()
    return -(((x * x).sum(1, keepdim=True) - 2.0 * (x @ e.t())) + ee[None, :])


def bound(x, embed, kernel=1):
    """Per-(row, column) bound on |kernel distance - distances()| for a correct kernel (module docstring)."""
    x, e = x.double(), embed.double()
    xx, ee = (x * x).sum(1), (e * e).sum(1)
    ax = x.abs() @ e.abs().t()
    b = C * ULP * (xx[:, None] + 2.0 * ax + ee[None, :])
    if kernel == 0:
        fin = x[torch.isfinite(x).all(1)]
        amax_x = float(fin.abs().max()) if fin.numel() else 0.0
        amax_x, amax_e = max(amax_x, 1.0), max(float(e.abs().max()), 1.0)        # (an operand stored unscaled, as the plans' activations are: 2^-36 itself)
        b = b + 2.0 * G.TOL * ax + 2.0 ** -35 * (amax_x * e.abs().sum(1)[None, :] + amax_e * x.abs().sum(1)[:, None])
    return b


def column_groups(embed):
    """[bins] id of each column's set of bit-identical codebook rows."""
    _u, inv = torch.unique(embed.contiguous().view(torch.int32), dim=0, return_inverse=True)
    return inv


class Ref:
    """distances, bound, duplicate groups and the rows fp32 cannot order, computed once per case and shared by the checks."""

    def __init__(self, x, embed, kernel, ee=None):
        self.kernel, self.rows, self.bins = kernel, x.shape[0], embed.shape[0]
        self.nan_rows = torch.isnan(x).any(1)
        self.ovf_rows = ~self.nan_rows & ((x.double() ** 2).sum(1) > FLT_MAX)
        self.plain = ~(self.nan_rows | self.ovf_rows)
        assert kernel == 1 or not bool(self.ovf_rows.any()), "the split-f16 form holds no such row"
        self.d = distances(x, embed, ee)
        self.b = bound(x, embed, kernel)
        self.gid = column_groups(embed)


def _slabs(t, width, nparts, fill):
    rows, bins = t.shape
    out = torch.full((rows, nparts * width), fill, dtype=t.dtype)
    out[:, :bins] = t
    return out.reshape(rows, nparts, width)


def _first(mask):
    """Lowest index along the last axis at which mask holds (its length where none does); argmax promises no such order."""
    n = mask.shape[-1]
    return torch.where(mask, torch.arange(n), torch.full((), n, dtype=torch.long)).amin(-1)


def _check_slabs(ref, width, nparts, idx, val, what):
    """The four conditions of a (value, index) candidate per (row, slab of `width` columns); val None: conditions 2 to 4 only.
    Returns the worst |val - maximum| / bound."""
    rows, bins = ref.rows, ref.bins
    idx = torch.as_tensor(idx).reshape(rows, nparts).long()
    start = torch.arange(nparts) * width
    filled = (start < bins)[None, :].expand(rows, nparts)
    if val is not None:
        val = torch.as_tensor(val).reshape(rows, nparts).double()
        empty = ~filled
        assert bool((val[empty] == -math.inf).all()) and bool((idx[empty] == NO_INDEX).all()), f"{what}: an empty slab must read (-inf, 0x7fffffff)"
    # rows fp32 cannot order
    nanp = ref.nan_rows[:, None] & filled
    assert bool((idx[nanp] == NO_INDEX).all()), f"{what}: a NaN row must select nothing"
    ovfp = ref.ovf_rows[:, None] & filled
    assert bool((idx[ovfp] == start[None, :].expand(rows, nparts)[ovfp]).all()), f"{what}: a row of -inf distances must name the slab's first column"
    if val is not None:
        assert bool((val[nanp | ovfp] == -math.inf).all()), f"{what}: NaN and overflowing rows must read -inf"
    ok = ref.plain[:, None] & filled
    d = _slabs(ref.d, width, nparts, -math.inf)
    b = _slabs(ref.b, width, nparts, 0.0)
    g = _slabs(ref.gid[None, :].expand(rows, bins), width, nparts, -1)
    top, targ = d.max(-1)                                           # (any maximal index: only its bound and duplicate set are read)
    btop = b.gather(-1, targ[..., None])[..., 0]
    gtop = g.gather(-1, targ[..., None])[..., 0]
    # 2: inside the slab
    local = idx - start[None, :]
    ncol = (bins - start).clamp(max=width)[None, :]
    inside = (local >= 0) & (local < ncol)
    assert bool(inside[ok].all()), f"{what}: {int((~inside & ok).sum())} indices outside their slab, e.g. {idx[~inside & ok][:4].tolist()}"
    lc = local.clamp(0, width - 1)
    dsel = d.gather(-1, lc[..., None])[..., 0]
    bsel = b.gather(-1, lc[..., None])[..., 0]
    # 3: the chosen column is within 2 bound of the maximum
    near = (top - dsel) <= btop + bsel
    assert bool(near[ok].all()), (f"{what}: {int((~near & ok).sum())} candidates further than 2 bound from the maximum, worst "
                                  f"{float(((top - dsel) / (btop + bsel))[ok].max()):.3g} x")
    # 4: no column outside the maximum's duplicate set within 2 bound of it -> exactly the lowest maximising index
    same = g == gtop[..., None]
    threat = ~same & (d + b >= (top - btop)[..., None])
    strict = ~threat.any(-1) & ok
    want = _first(same)                                             # first column of the duplicate set inside the slab
    wrong = strict & (local != want)
    assert not bool(wrong.any()), (f"{what}: {int(wrong.sum())} of {int(strict.sum())} decidable candidates are not the lowest maximising "
                                   f"index, e.g. (row, slab, got, want) {[(int(r), int(p), int(idx[r, p]), int(want[r, p] + start[p])) for r, p in wrong.nonzero()[:4]]}")
    frac = 0.0
    if val is not None:
        # 1: the value is within the bound of the maximum (of the maximum's own bound below it, of the chosen column's above)
        err = (val - top).abs() / torch.maximum(btop, bsel)
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
        frac = float(err[ok].max()) if bool(ok.any()) else 0.0
        assert frac <= 1.0, f"{what}: {int((err > 1.0)[ok].sum())} values outside the bound, worst {frac:.3g} x"
    return frac, int(strict.sum()), int(ok.sum())


def check_parts(pval, pidx, form, x, embed, kernel=None, ee=None, ref=None, what="parts"):
    """Every row and every part against the slab the part covers (part q: columns [q WN, (q + 1) WN), WN = BN / waves_n).
    Returns (worst |pval - slab maximum| / bound, decidable candidates, candidates of ordinary rows)."""
    ref = ref or Ref(x, embed, kernel, ee)
    wn = form.BN // form.waves_n
    assert form.nparts * wn >= ref.bins and (form.nparts - 2) * wn < ref.bins, (form.nparts, wn, ref.bins)
    return _check_slabs(ref, wn, form.nparts, pidx, pval, what)


def check_codes(codes, x, embed, kernel=None, ee=None, ref=None, what="codes"):
    """Conditions 3 and 4 over the whole row; NaN and overflowing rows: code 0.  Returns (decidable rows, ordinary rows)."""
    ref = ref or Ref(x, embed, kernel, ee)
    codes = torch.as_tensor(codes).reshape(ref.rows).long()
    odd = ref.nan_rows | ref.ovf_rows
    assert bool((codes[odd] == 0).all()), f"{what}: a NaN or overflowing row must give code 0"
    assert bool(((codes >= 0) & (codes < ref.bins)).all()), f"{what}: a code outside the codebook"
    shown = torch.where(ref.nan_rows, torch.full_like(codes, NO_INDEX), codes)      # (the whole row as one slab starting at 0)
    _f, strict, ok = _check_slabs(ref, ref.bins, 1, shown, None, what)
    return strict, ok


def check_feat(feat, codes, embed, what="feat"):
    """feat [B][D][L] must be embed[codes] [B][L][D] transposed, bit for bit: a copy, so the tolerance is zero."""
    feat = torch.as_tensor(feat)
    B, D, L = feat.shape
    want = embed[torch.as_tensor(codes).reshape(B, L).long()].transpose(1, 2).contiguous()
    same = feat.contiguous().view(torch.int32) == want.view(torch.int32)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} words differ from embed[codes], e.g. (b, d, t) {(~same).nonzero()[:3].tolist()}"


def undecidable(ref):
    """(rows whose float64 top-2 margin outside the maximum's duplicate set is at most 2 bound, ordinary rows): the only rows
    allowed more than one answer."""
    # (the float64 product itself need not give bit-identical columns equal distances: the duplicate set decides, as in the checks)
    lowest = _first(ref.gid[None, :] == ref.gid[torch.nan_to_num(ref.d, nan=0.0).argmax(-1)][:, None])
    strict, ok = check_codes(lowest * ref.plain, None, None, ref=ref)
    return ok - strict, ok


# ------------------------------------------------------------------------------------------------ input builders
def tie_sets(bins, bn, wn):
    """Column sets that must tie, one per merge level of the argmax epilogue and of vq_finalize, from the tile geometry: inside a
    lane's 4-column run, the lane pair (n, n + 4), 8- and 16-column groups, 32-column MFMA tiles, the wave slab, the block tile,
    the finalize lanes (part q against q + 8), first against last column, and a three-way tie over three block tiles.  Sets
    that do not fit the codebook are left out; no column is used twice."""
    want = [(1, 2), (8, 12), (3, 11), (13, 29), (5, 37), (31 + 32, 64), (wn - 1, wn), (10, wn + 4), (bn - 1, bn), (50, bn + 58),
            (wn + 8, 9 * wn + 8), (bn + 17, bn + 17 + 8 * wn), (0, bins - 1), (bn + 2 * wn + 1, 3 * bn + 3, 5 * bn + wn + 7),
            (2 * bn - 1, 2 * bn), (bins - 3, bins - 2)]
    used, out = set(), []
    for s in want:
        s = tuple(sorted(set(s)))
        if len(s) < 2 or s[0] < 0 or s[-1] >= bins or used & set(s):
            continue
        used |= set(s)
        out.append(s)
    return out, used


def near_pairs(bins, bn, wn, used):
    """Column pairs (a < b) for the near-tie rows, across the same boundaries, away from the duplicated columns."""
    want = [(6, 7), (20, 24), (40, 48), (26 + 32, 26 + 64), (wn - 2, wn + 1), (bn - 2, bn + 1), (wn + 31, 9 * wn + 31), (bn + 40, 2 * bn + 40),
            (2, bins - 2), (3 * bn - 1, 3 * bn)]
    out = []
    for a, b in want:
        if 0 <= a < b < bins and not used & {a, b}:
            used |= {a, b}
            out.append((a, b))
    return out


def near_tie_row(embed, a, b, kernel, m=M_TIE):
    """fp32 x = (e_a + e_b) / 2 + s (e_a - e_b) whose float64 margin d[a] - d[b], computed from the rounded x, is m times
    (bound[a] + bound[b]) / 2: a wins."""
    ea, eb = embed[a].double(), embed[b].double()
    den = 2.0 * float(((ea - eb) ** 2).sum())                       # d[a] - d[b] = 2 s |e_a - e_b|^2
    s = 0.0
    for _ in range(8):
        x = ((ea + eb) / 2 + s * (ea - eb)).float()
        pair = embed[[a, b]]
        d = distances(x[None], pair)[0]
        bb = bound(x[None], pair, kernel)[0]
        target = m * float(bb.sum()) / 2
        s += (target - float(d[0] - d[1])) / den
    return x


class Case:
    """One seeded problem: x [rows][D], embed [bins][D] and what each designed row must give (want: row -> code)."""

    def __init__(self, bins, D, rows, kernel, seed, special=True, scale=0.6, designed=True):
        bn, wn, _np = geometry(kernel, bins)
        gen = torch.Generator().manual_seed(seed)
        embed = torch.randn(bins, D, generator=gen) * 0.6
        sets, used = tie_sets(bins, bn, wn)
        for s in sets:
            for c in s[1:]:
                embed[c] = embed[s[0]]                               # exact duplicates: every tie must resolve to s[0]
        x = torch.randn(rows, D, generator=gen) * scale
        designed = []
        for s in sets:                                               # distance 0 to every copy, far from everything else
            designed += [(embed[s[0]].clone(), s[0]), (embed[s[-1]] * 1.0, s[0])]
        n_dup = len(designed)
        for a, b in near_pairs(bins, bn, wn, set(used)):             # the winner in both orders
            designed += [(near_tie_row(embed, a, b, kernel), a), (near_tie_row(embed, b, a, kernel), b)]
        specials = []
        if special and rows >= 8:
            specials = [("zero", torch.zeros(D)), ("nan", torch.full((D,), math.nan))]
            if kernel == 1:
                specials.append(("overflow", torch.where(torch.arange(D) % 2 == 0, 1.5e19, -1.5e19)))
        self.want, self.special = {}, {}
        r = 0
        for name, row in specials:                                   # each between two random rows
            r += 1
            x[r] = row
            self.special[name] = r
            r += 1
        self.near_rows = []
        for i, (row, code) in enumerate(designed[:max(0, rows - r - 1)] if designed else []):
            r += 1
            x[r] = row
            self.want[r] = code
            if i >= n_dup:
                self.near_rows.append(r)
        self.x, self.embed, self.kernel, self.bins, self.D, self.rows = x, embed, kernel, bins, D, rows
        self.sets = sets
        self._ref = {}

    def ref(self, ee=None):
        key = None if ee is None else "ee"
        if key not in self._ref:
            self._ref[key] = Ref(self.x, self.embed, self.kernel, ee)
        return self._ref[key]

    def check_designed(self, codes, what="designed rows", near=True):
        """near = False: the exact ties and the special rows only (the near-tie rows are placed against the float64 |e|^2; with
        another table handed in, check_codes decides which of them still have one answer)."""
        codes = torch.as_tensor(codes).reshape(-1)
        bad = [(r, int(codes[r]), c) for r, c in self.want.items() if int(codes[r]) != c and (near or r not in self.near_rows)]
        assert not bad, f"{what}: (row, got, want) {bad[:6]}"
        for name, r in self.special.items():
            if name != "zero":
                assert int(codes[r]) == 0, f"{what}: the {name} row gave code {int(codes[r])}"


def host_serial_ee(embed):
    """weights.cpp's table: one serial fp32 chain per codebook row."""
    e = embed.float()
    s = torch.zeros(e.shape[0], dtype=torch.float32)
    for c in range(e.shape[1]):
        s = s + e[:, c] * e[:, c]
    return s
