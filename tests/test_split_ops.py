"""GPU: the format converters under every S32 operand - split_s32_kernel, unsplit_s32_kernel, amax_bits_kernel and
pow2_scale_kernel (gemm16s.hip) - through wt_split_probe, which calls the launchers the loader, the plans and the single-stage
entry points call, against the numpy emulation and the float64 bound of tests/weights_ref.py; and wt_linear's per-tensor
scales at the ends of fp32's exponent range."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_ref as G, weights_ref as W

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel words either side of an output
RANGE_BIT = 2                  # WT_STATUS_BIT_RANGE


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _probe(op, x, out, n, b=None, nb=0, scale=None, bits=None, inv_scale=1.0, status=None):
    from wavtokenizer_amd._capi import lib, check, WtSplitDesc
    d = WtSplitDesc(size=ctypes.sizeof(WtSplitDesc), op=op, n=n, nb=nb, x=x.data_ptr(), b=b.data_ptr() if b is not None else None,
                    out=out.data_ptr(), scale=scale.data_ptr() if scale is not None else None,
                    bits=bits.data_ptr() if bits is not None else None, inv_scale=inv_scale, status=status.data_ptr() if status is not None else None)
    check(lib.wt_split_probe(ctypes.byref(d), None), "wt_split_probe")
    torch.cuda.synchronize()


EDGES = [0.0, -0.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65503.9, 2.0 ** -36, 2.0 ** -37,
         -(1 + 2.0 ** -11), -(2.0 ** -25), 2.0 ** -120, -1.5 * 2.0 ** -118]
OVER = {"none": [], "65519.9": [65519.9], "65520": [65520.0], "-65520": [-65520.0], "nan": [float("nan")], "+inf": [float("inf")],
        "-inf": [float("-inf")], "all": [65519.9, 65520.0, float("nan"), float("inf"), float("-inf")]}


def _values(n, over, seed):
    rng = np.random.default_rng(seed)
    v = (np.exp2(rng.uniform(-40, 15, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    t = np.array(EDGES + OVER[over], np.float32)
    v[:t.size] = t                               # (n >= 32 holds the whole table)
    v[-1] = np.float32(-(2.0 ** -25))            # an edge value in the last element too
    return v


def _run_split(v, sc):
    """-> (uint16 words, status word); sentinels either side of the output checked."""
    n = v.size
    x = torch.from_numpy(v).cuda()
    buf = torch.full((n + 2 * GUARD,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    scale = torch.tensor([sc, 7.0, 7.0, 7.0], dtype=torch.float32, device="cuda") if sc is not None else None
    _probe(0, x, buf[GUARD:], n, scale=scale, status=status)
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == 0x5a5a5a5a) and np.all(host[-GUARD:] == 0x5a5a5a5a), "split wrote outside its output"
    st = status.cpu().numpy()
    assert np.all(st[1:] == 0)
    return host[GUARD:-GUARD].copy().view(np.uint16), int(st[0]), buf


def _check_split(v, sc, words, status, what):
    s = 1.0 if sc is None else sc
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p32 = v * np.float32(s)
    p64 = v.astype(np.float64) * s
    want = W.split_emulate(p32).view(np.uint16).reshape(-1, 2, 32)
    got = words.reshape(-1, 2, 32)
    # a product that is an fp32 subnormal is checked against the bound only: the compiler may contract x * sc - h
    sub = ((p64 != 0) & (np.abs(p64) < 2.0 ** -126)).reshape(-1, 32)
    for half in (0, 1):
        g, w = got[:, half, :], want[:, half, :]
        bad = ~W.words_match(g, w, hi=np.full(g.shape, half == 0)) & ~sub
        assert not bad.any(), (what, "hi" if half == 0 else "lo", "first differing element", int(np.flatnonzero(bad.reshape(-1))[0]))
    ok = np.isfinite(p64) & (np.abs(p64) < 65504.0)
    err = np.abs(p64 - W.split_value(words))[ok] / W.split_bound(p64[ok])
    assert err.max() <= 1.0, (what, "worst err / bound", float(err.max()))
    # common.h range_report: the bit is raised when the largest |value converted|, NaNs ignored (amax1 is an fmaxf), is >= 65504
    m = np.abs(p32[~np.isnan(p32)])
    flag = bool(m.size and m.max() >= np.float32(65504.0))
    assert status == (RANGE_BIT if flag else 0), (what, "status", status, "expected the range bit" if flag else "expected 0")
    return float(err.max())


SCALES = [None, 2.0 ** -13, 2.0 ** 9]


@pytest.mark.parametrize("sc", SCALES, ids=["unscaled", "2^-13", "2^9"])
@pytest.mark.parametrize("n", [32, 96, 4096, 8192 * 256 + 64])
def test_split_and_unsplit(n, sc):
    """Every word of the split equals the emulation's, every finite in-range value meets the float64 bound, the status word
    carries the range bit by range_report's rule, with and without the over-range rows of the edge table; the last size is
    past the 8192-block cap, so the grid-stride loop wraps.  Then unsplit on that output: bit-equal to fp32
    (hi + lo / 2048) * inv_scale, and unsplit(split(x)) within the bound of x.  (The one word that is not the emulation's: the hi
    half of -0 is +0, weights_ref.words_match.)"""
    worst = 0.0
    for over in ("none", "all"):
        v = _values(n, over, seed=n + (0 if over == "none" else 1))
        words, status, buf = _run_split(v, sc)
        worst = max(worst, _check_split(v, sc, words, status, (n, sc, over)))
        s = 1.0 if sc is None else sc
        for inv in sorted({1.0, 2.0 ** 13, 2.0 ** -9, 1.0 / s}):
            out = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
            out[:GUARD] = 12345.0
            out[-GUARD:] = 12345.0
            _probe(1, buf[GUARD:], out[GUARD:], n, inv_scale=inv)
            host = out.cpu().numpy()
            assert np.all(host[:GUARD] == 12345.0) and np.all(host[-GUARD:] == 12345.0), "unsplit wrote outside its output"
            got, want = host[GUARD:-GUARD], W.split_value_f32(words, inv)
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), (n, sc, inv, "first differing element", int(np.flatnonzero(~same)[0]))
            if inv == 1.0 / s:
                p64 = v.astype(np.float64) * s
                ok = np.isfinite(p64) & (np.abs(p64) < 65504.0)
                err = np.abs(v.astype(np.float64) - got.astype(np.float64))[ok] / (W.split_bound(p64[ok]) / s)
                assert err.max() <= 1.0, (n, sc, "round trip: worst err / bound", float(err.max()))
    print(f"split n={n} scale={sc}: worst err / bound {worst:.4f}")


@pytest.mark.parametrize("sc", SCALES, ids=["unscaled", "2^-13", "2^9"])
@pytest.mark.parametrize("over", [k for k in OVER if k not in ("none", "all")])
def test_split_status_per_edge_value(over, sc):
    """One over-range row of the table at a time, in magnitudes that are otherwise below 2^6 (so that no scale here moves a
    random value past the range): the bit follows range_report's rule - raised for |v sc| >= 65504 and for an infinity, not for a
    NaN, which propagates into the words by itself."""
    v = _values(96, over, seed=5)
    big = np.abs(v) >= 64.0
    big[:len(EDGES) + len(OVER[over])] = False
    v[big] = np.float32(0.5)
    words, status, _buf = _run_split(v, sc)
    _check_split(v, sc, words, status, (over, sc))
    if over == "nan":
        hi, _lo = W.split_halves(words)
        assert np.isnan(hi[len(EDGES)])
        assert status == (RANGE_BIT if sc == 2.0 ** 9 else 0)          # (65503.9 * 2^9 is over the range; the NaN raises nothing)


# ------------------------------------------------------------------------------------------------ launch_pow2_scales
NB = 2048 * 256 + 32           # past the 2048-block cap of amax_bits_kernel


def _scale_rule(mx):
    """pow2_scale_kernel's comment: the maximum is brought into [1, 2) by a normal power of two, or the scale is 1 (zero,
    subnormal, inf / NaN, or a maximum so large that the scale would not be normal: biased exponent >= 253)."""
    bits = int(np.float32(abs(mx)).view(np.uint32))
    e = (bits >> 23) & 0xff
    return bits, (1.0 if e == 0 or e >= 253 else 2.0 ** (127 - e))


def _run_scales(a, b):
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    bits = torch.full((4,), 0x55, dtype=torch.int32, device="cuda")
    out = torch.full((5,), 9.0, dtype=torch.float32, device="cuda")
    _probe(2, ta, out, a.size, b=tb, nb=b.size, bits=bits)
    o, bt = out.cpu().numpy(), bits.cpu().numpy()
    assert o[3] == 9.0 and o[4] == 9.0 and bt[2] == 0x55 and bt[3] == 0x55
    return bt[:2].view(np.uint32), o[:3]


def _noise(n, mx, seed):
    """n values of both signs, every magnitude at most half of |mx| (0 when mx is 0 or not finite)."""
    rng = np.random.default_rng(seed)
    top = abs(mx) if np.isfinite(mx) else 1.0
    with np.errstate(under="ignore"):
        return (rng.uniform(-0.5, 0.5, n) * top).astype(np.float32)


EXP_CASES = {"subnormal": -1.5 * 2.0 ** -130, "e1": 1.25 * 2.0 ** -126, "e126": -0.75, "e127": 1.0, "e128": -3.0, "e252": 1.5 * 2.0 ** 125,
             "e253": -1.25 * 2.0 ** 126, "e254": 1.5 * 2.0 ** 127, "inf": float("-inf"), "zero": 0.0}


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("case", list(EXP_CASES))
def test_pow2_scales_exponent_table(case, slot):
    """The maximum of one tensor at every corner of the exponent range, the other tensor moderate (5.5, negative, in its last
    element), in either slot and so in both sizes: 32 elements and 2048 * 256 + 32.  Both scales follow the kernel's comment
    and out[2] is exactly 1 / (scale_a * scale_b), finite and normal - which it is because the other tensor is moderate:
    test_pow2_scales_both_tensors_at_one_corner has the two pairs where fp32 cannot hold that factor."""
    mx = EXP_CASES[case]
    sizes = (32, NB) if slot == 0 else (NB, 32)
    t = [None, None]
    t[slot] = _noise(sizes[slot], mx, 1)
    t[slot][sizes[slot] // 3] = np.float32(mx)
    t[1 - slot] = _noise(sizes[1 - slot], 5.5, 2)
    t[1 - slot][-1] = np.float32(-5.5)
    bits, out = _run_scales(t[0], t[1])
    want = [None, None]
    want[slot], want[1 - slot] = _scale_rule(mx), _scale_rule(5.5)
    for i in (0, 1):
        assert int(bits[i]) == want[i][0], (case, i, hex(int(bits[i])), hex(want[i][0]))
        assert float(out[i]) == want[i][1], (case, i, float(out[i]), want[i][1])
    sc = float(out[slot])
    assert sc == 1.0 or 1.0 <= abs(mx) * sc < 2.0
    if case not in ("subnormal", "e253", "e254", "inf", "zero"):
        assert sc != 1.0 or case == "e127"
    tiny = float(np.finfo(np.float32).tiny)
    assert float(out[2]) == 1.0 / (float(out[0]) * float(out[1])) and tiny <= float(out[2]) < float("inf")


@pytest.mark.parametrize("case,want", [("e1", 0.0), ("e252", float("inf"))])
def test_pow2_scales_both_tensors_at_one_corner(case, want):
    """out[2] is the fp32 product (1 / scale_a) * (1 / scale_b): exactly 1 / (scale_a scale_b), finite and normal, while that
    lies inside fp32's normal range, 2^-126 <= 1 / (scale_a scale_b) < 2^128.  With both maxima at biased exponent 1 the scales
    are 2^126 each and 2^-252 rounds to 0; with both at 252 they are 2^-125 each and 2^250 is inf.  (A product of two such
    tensors is outside fp32 itself: the scales are right, the restoring factor cannot be.)"""
    mx = EXP_CASES[case]
    a, b = _noise(32, mx, 5), _noise(NB, mx, 6)
    a[3], b[NB // 2] = np.float32(mx), np.float32(-mx)
    bits, out = _run_scales(a, b)
    rule = _scale_rule(mx)
    assert int(bits[0]) == rule[0] == int(bits[1]) and float(out[0]) == rule[1] == float(out[1])
    assert float(out[2]) == want


def test_pow2_scales_finds_the_maximum_in_every_lane():
    """The maximum planted once in each lane of one wave of a block in the middle of the large tensor, and once in its last
    element; a NaN beside it is ignored (fmaxf); an all-NaN tensor gives scale 1."""
    base = _noise(NB, 1.0, 3)
    small = _noise(32, 1.0, 4)
    small[7] = np.float32(0.9)
    wave0 = 256 * 1031 + 64
    for pos in list(range(wave0, wave0 + 64)) + [NB - 1]:
        b = base.copy()
        mx = np.float32(-6.5 if pos % 2 else 6.5)
        b[pos] = mx
        b[pos - 1 if pos == NB - 1 else pos + 1] = np.float32("nan")
        bits, out = _run_scales(small, b)
        assert int(bits[1]) == int(np.float32(6.5).view(np.uint32)) and float(out[1]) == 0.25, (pos, hex(int(bits[1])), float(out[1]))
        assert int(bits[0]) == int(np.float32(0.9).view(np.uint32)) and float(out[0]) == 2.0 and float(out[2]) == 2.0
    bits, out = _run_scales(np.full(32, np.nan, np.float32), base)
    assert int(bits[0]) == 0 and float(out[0]) == 1.0


# ------------------------------------------------------------------------------------------------ wt_linear
@pytest.mark.parametrize("k", [-126, -100, 100, 125])
def test_linear_s32_operand_scale_corners(k):
    """wt_linear modes 2 (fp32 out) and 3 (S32 out) with the weights times 2^k and the activations times 2^-k (2^120 against
    2^-126, so that no activation leaves fp32), at (M, N, K) = (33, 32, 64), against float64 with gemm_ref's tolerance: TOL on
    sum |x w| + |b| and one fp32 rounding of the result.  Where both operands are scaled (every k but -126) the absolute floor
    of the two scaled splits is added: each operand, brought into [1, 2), is within 2^-36 of its split, so the accumulator moves
    by at most K (2 2^-36 + 2 2^-36) = K 2^-34 in scaled units, K 2^-34 / (scale_x scale_w) in the caller's.

    k = -126 is a LIMITATION of the single-stage entry points, asserted as what it is and not as a met bound: the weights are
    fp32 subnormals, pow2_scale_kernel's guard leaves their scale at 1, every one of them splits to hi = lo = 0, and the call
    returns the bias alone - the whole product x . w (about 2^-6 here) is lost, and wt_linear has no status word to say so.  The
    plans do not share it: a model weight with such a maximum is not split at all (add_s32 clears s32_ok)."""
    from wavtokenizer_amd._capi import lib, check
    M, N, K = 33, 32, 64
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=gen) * 2.0 ** (120 if k == -126 else -k)
    w = torch.randn(N, K, generator=gen) / K ** 0.5 * 2.0 ** k
    b = torch.randn(N, generator=gen) * 2.0 ** (-6 if k == -126 else 0)
    assert torch.isfinite(x).all() and torch.isfinite(w).all() and float(w.abs().max()) > 0
    ref = x.double() @ w.double().t() + b.double()
    mag = x.double().abs() @ w.double().abs().t() + b.double().abs()
    sx, sw = _scale_rule(float(x.abs().max()))[1], _scale_rule(float(w.abs().max()))[1]
    assert (sw == 1.0) == (k == -126) and sx != 1.0
    bound = G.TOL * mag + G.ULP * ref.abs()
    if k != -126:
        bound = bound + K * 2.0 ** -34 / (sx * sw)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    ws = torch.zeros(4 * (M + N) * K + 4096, dtype=torch.uint8, device="cuda")
    for mode in (2, 3):
        y = torch.full((M, N), float("nan"), device="cuda")
        check(lib.wt_linear(_ptr(xd), _ptr(wd), _ptr(bd), _ptr(y), M, N, K, mode, _ptr(ws), None), "wt_linear")
        torch.cuda.synchronize()
        if mode == 3:
            got = G.decode_s32_rows(y.cpu().contiguous().view(torch.int16), M, N)
            bnd = bound + G.S32_ENC * ref.abs() + G.ABS_FLOOR
        else:
            got, bnd = y.cpu().double(), bound
        n_bad, worst, finite = G.check(got, ref, bnd)
        print(f"wt_linear 2^{k} mode {mode}: worst err / bound {worst:.4g}, {n_bad} of {M * N} outside")
        assert finite
        if k != -126:
            assert n_bad == 0, (k, mode, n_bad, worst)
        else:
            # the documented loss: the product is dropped whole, the result is the bias (re-encoded in mode 3), and it does NOT
            # meet the float64 bound
            lost = b.double().expand(M, N)
            assert n_bad > 0 and float((ref - lost).abs().max()) > 2.0 ** -10, "the guard case no longer loses the product: assert the bound instead"
            tol = G.S32_ENC * lost.abs() + G.ABS_FLOOR if mode == 3 else torch.zeros_like(lost)
            assert bool(((got - lost).abs() <= tol).all()), "the guard case returns something other than the bias"
