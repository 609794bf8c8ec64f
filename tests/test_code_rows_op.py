"""code_rows_kernel / code_rows_mixed_kernel (csrc/ops_kernel.inc), the first step of the decode-from-codes plans, one launch at
a time through wt_op_probe (WT_OP_CODE_ROWS).  The reference is numpy on the host: per frame acc = 0.f, acc += row_k for
k = 0 .. K - 1 in float32, the order of codes_to_features_kernel.  fp32 rows must be those bits; S32 rows must decode
(tests/gemm_ref.decode_s32_rows) to the split of those bits, hi = f16(v), lo = f16((v - hi) * 2048).  A code outside [0, bins)
gives a NaN row and sets the bad-index word, never the status word; the length-aware twin writes zero rows past a clip's length
and never looks at the codes there."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -559038737                # 0xDEADBEEF


class Out:
    """A device output of n fp32 words between two guard runs, pre-filled with a sentinel that no result holds."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32).cuda()
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def host(self):
        h = self.buf.cpu()
        assert bool((h[:GUARD] == SENT).all()) and bool((h[GUARD + self.n:] == SENT).all()), "guard words overwritten"
        return h[GUARD:GUARD + self.n]

    def untouched(self):
        return bool((self.buf.cpu() == SENT).all())


def _desc(**kw):
    from wavtokenizer_amd import _capi
    d = _capi.WtOpDesc()
    d.size = ctypes.sizeof(d)
    d.op = _capi.WT_OP_CODE_ROWS
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def probe(**kw):
    from wavtokenizer_amd import _capi
    f = _capi.WtOpForm()
    d = _desc(**kw)
    rc = _capi.lib.wt_op_probe(ctypes.byref(d), ctypes.byref(f), None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    return _capi.WT_OPK_NAMES[f.kernel], f


@functools.lru_cache(maxsize=None)
def _table(bins, C):
    """Three codebooks of `bins` rows (one array, shared and never modified), every 97th entry -0.0f; and its device copy."""
    rng = np.random.default_rng(bins + C)
    t = rng.standard_normal((3 * bins, C)).astype(np.float32)
    t.reshape(-1)[::97] = -0.0
    t.setflags(write=False)
    return t, torch.from_numpy(t.copy()).cuda()


def _codes(K, B, L, bins, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, bins, size=(K, B, L), dtype=np.int64)
    c[0, 0, 0] = 0
    c[-1, -1, -1] = bins - 1
    return c


def ref_rows(codes, table, bins):
    """[K][B][L] codes -> float32 [B][L][C]: plain float32 adds in codebook order on a zero accumulator; NaN for a bad code."""
    K, B, L = codes.shape
    acc = np.zeros((B, L, table.shape[1]), np.float32)
    for k in range(K):
        ok = (codes[k] >= 0) & (codes[k] < bins)
        rows = table[k * bins + np.where(ok, codes[k], 0)]
        acc = acc + np.where(ok[..., None], rows, np.float32("nan"))
    assert acc.dtype == np.float32
    return acc


def split_ref(v):
    """float32 values -> float64 value of their S32 form, hi + lo / 2048 with hi = f16(v), lo = f16((v - hi) * 2048)."""
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.astype(np.float64) + lo.astype(np.float64) / 2048.0


def _same(got_words, ref, s32, what):
    """got_words: the int32 words of [rows][C] output slots; ref float32 [rows][C]."""
    rows, C = ref.shape
    if s32:
        got = G.decode_s32_rows(got_words.contiguous().view(torch.int16).reshape(-1), rows, C).numpy()
        want = split_ref(ref)
        assert np.array_equal(got, want, equal_nan=True), what
    else:
        assert np.array_equal(got_words.numpy().view(np.uint32).reshape(rows, C), ref.view(np.uint32)), what


def _run(codes, bins, C, s32, lengths=None):
    """One probe launch: (kernel name, form, output words [B * L * C], bad word, status word)."""
    K, B, L = codes.shape
    _t, td = _table(bins, C)
    cd = torch.from_numpy(codes).cuda()
    y = Out(B * L * C)
    bad = torch.zeros(4, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    kw = dict(B=B, L=L, C=C, k=K, n=bins, out_s32=s32, x=cd.data_ptr(), p0=td.data_ptr(), y=y.ptr, y2=bad.data_ptr(),
              status=status.data_ptr())
    lens = None
    if lengths is not None:
        lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
        kw["lengths"] = lens.data_ptr()
    name, f = probe(**kw)
    return name, f, y.host(), int(bad[0]), int(status[0])


@pytest.mark.parametrize("s32", [0, 1])
@pytest.mark.parametrize("bins", [7, 4096])
@pytest.mark.parametrize("C", [64, 512])
def test_rows_are_the_float32_sum_in_codebook_order(C, bins, s32):
    table, _td = _table(bins, C)
    for B in (1, 3):
        for L in (1, 5, 33):              # fewer frames than a workgroup holds, a partial last workgroup, several workgroups
            for K in (1, 3):
                codes = _codes(K, B, L, bins, seed=B * 100 + L * 3 + K)
                name, f, words, bad, status = _run(codes, bins, C, s32)
                what = (C, bins, s32, B, L, K)
                assert name == "code_rows" and f.variant == (C + 255) // 256, what
                assert (f.grid_x, f.grid_y, f.grid_z, f.block, f.lds) == ((B * L + 3) // 4, 1, 1, 256, 0), what
                _same(words, ref_rows(codes, table, bins).reshape(B * L, C), s32, what)
                assert bad == 0 and status == 0, what


def test_negative_zero_entries_come_out_as_positive_zero():
    """acc = 0.f + (-0.f) is +0.f: with one codebook the kernel must not copy the row."""
    table, _td = _table(7, 64)
    codes = np.zeros((1, 1, 1), np.int64)
    assert np.signbit(table[0, 0]) and table[0, 0] == 0
    _name, _f, words, _bad, _status = _run(codes, 7, 64, 0)
    assert int(words[0]) == 0                              # (the bits of +0.0f; -0.0f is 0x80000000)
    _same(words, ref_rows(codes, table, 7).reshape(1, 64), 0, "k1")


@pytest.mark.parametrize("s32", [0, 1])
@pytest.mark.parametrize("C", [64, 512])
def test_bad_indices_give_nan_rows_and_the_bad_word_only(C, s32):
    bins, K, B, L = 7, 3, 3, 5
    table, _td = _table(bins, C)
    codes = _codes(K, B, L, bins, seed=5)
    where = {(0, 0, 1): -1, (1, 1, 4): bins, (2, 2, 2): 2 ** 40}       # (k, b, t) -> code: one frame each
    for pos, v in where.items():
        codes[pos] = v
    name, _f, words, bad, status = _run(codes, bins, C, s32)
    assert name == "code_rows"
    ref = ref_rows(codes, table, bins)
    nan_rows = np.isnan(ref).all(-1)
    assert int(nan_rows.sum()) == 3 and all(nan_rows[b, t] for _k, b, t in where)
    assert not np.isnan(ref[~nan_rows]).any()
    if s32:
        got = G.decode_s32_rows(words.contiguous().view(torch.int16).reshape(-1), B * L, C).numpy().reshape(B, L, C)
    else:
        got = words.numpy().view(np.float32).reshape(B, L, C)
    assert np.array_equal(np.isnan(got), np.isnan(ref))      # exactly those rows, every element of them
    _same(words, ref.reshape(B * L, C), s32, "bad indices")   # every other row is exact
    assert bad == 1
    assert status == 0                                        # NaN does not raise the range bit


@pytest.mark.parametrize("s32", [0, 1])
@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("L", [5, 33])
def test_mixed_twin_writes_zero_rows_and_never_reads_past_a_length(L, C, s32):
    bins, K = 4096 if C == 512 else 7, 3
    lengths = [L, 1, 3]
    B = len(lengths)
    codes = _codes(K, B, L, bins, seed=L + C)
    staged = codes.copy()
    for b, Lb in enumerate(lengths):
        fill = np.where(np.arange(L - Lb) % 2 == 0, -1, 2 ** 62).astype(np.int64)
        staged[:, b, Lb:] = fill
    name, f, words, bad, status = _run(staged, bins, C, s32, lengths)
    assert name == "code_rows_mixed" and f.variant == (C + 255) // 256 and f.grid_x == (B * L + 3) // 4
    assert bad == 0 and status == 0
    got = words.reshape(B, L, C)
    for b, Lb in enumerate(lengths):
        own = np.ascontiguousarray(codes[:, b:b + 1, :Lb])
        sname, _f, swords, sbad, _st = _run(own, bins, C, s32)
        assert sname == "code_rows" and sbad == 0
        assert torch.equal(got[b, :Lb].reshape(-1), swords), (b, Lb)
        assert bool((got[b, Lb:] == 0).all()), (b, Lb)


@pytest.mark.parametrize("what,kw", [("C = 30", dict(C=30)), ("K = 0", dict(k=0)), ("null x", dict(x=None)),
                                     ("S32 with C = 36", dict(C=36, out_s32=1))])
def test_refused_descriptors_touch_nothing(what, kw):
    from wavtokenizer_amd import _capi
    bins = 7
    _t, td = _table(bins, 64)
    cd = torch.from_numpy(_codes(3, 3, 5, bins, seed=1)).cuda()
    y = Out(3 * 5 * 64)
    args = dict(B=3, L=5, C=64, k=3, n=bins, out_s32=0, x=cd.data_ptr(), p0=td.data_ptr(), y=y.ptr)
    args.update(kw)
    d = _desc(**args)
    assert _capi.lib.wt_op_probe(ctypes.byref(d), None, None) == _capi.WT_ERR_INVALID, what
    assert _capi.lib.wt_last_error()
    torch.cuda.synchronize()
    assert y.untouched(), what
