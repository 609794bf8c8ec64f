"""CPU-only halves of tests/test_gemm_epilogues.py: the per-element checker is tight enough to see the slips it is there
for, and wt_gemm_probe refuses bad descriptors before any HIP call (so these run on a host without a GPU)."""
import ctypes

import pytest
import torch

from tests import gemm_ref as G


def _problem(epi, M=40, N=64, K=96, seed=0):
    gen = torch.Generator().manual_seed(seed + 17 * epi)
    a = torch.randn(M, K, generator=gen, dtype=torch.float64)
    w = torch.randn(N, K, generator=gen, dtype=torch.float64) / K ** 0.5
    rows = M if epi == G.EPI_BIAS_ROW else N
    bias = torch.randn(rows, generator=gen, dtype=torch.float64)
    if epi == G.EPI_HEAD:
        bias = bias + 2.0
    R = torch.randn(M, N, generator=gen, dtype=torch.float64)
    gamma = torch.rand(N, generator=gen, dtype=torch.float64) + 0.5
    return dict(a=a, w=w, bias=bias, R=R, gamma=gamma, alpha=0.37, head_kb=N // 2)


def _result(p, epi, out, pro=G.PRO_NONE, drop_tile=False, acc_x2=False, no_bias=False, alpha_twice=False, gamma_twice=False,
            swap_head=False, dtype=torch.float64):
    """The epilogue's outputs from p in `dtype` arithmetic, optionally with one deliberate slip."""
    a = G.elu(p["a"]) if pro == G.PRO_ELU else p["a"]
    w = p["w"].clone()
    if drop_tile:
        w[:, 32:64] = 0
    acc = a.to(dtype) @ w.to(dtype).t()
    if acc_x2:
        acc = acc * 2
    acc = acc.double()
    bias = None if no_bias else p["bias"]
    gamma = p["gamma"] ** 2 if gamma_twice else p["gamma"]
    alpha = p["alpha"] ** 2 if alpha_twice else p["alpha"]
    outs, _ = G.epilogue(epi, out, acc, acc.abs(), bias=bias, R=p["R"], gamma=gamma, alpha=alpha, head_kb=p["head_kb"])
    if swap_head:
        kb = p["head_kb"]
        outs = [torch.cat([o[..., kb:], o[..., :kb]], -1) for o in outs]
    return [o.to(dtype).double() for o in outs]


def _slips(epi):
    s = ["drop_tile", "acc_x2"]
    if epi not in (G.EPI_SCALE,):
        s.append("no_bias")
    if epi == G.EPI_SCALE:
        s.append("alpha_twice")
    if epi == G.EPI_BIAS_GAMMA_RES:
        s.append("gamma_twice")
    if epi == G.EPI_HEAD:
        s.append("swap_head")
    return s


@pytest.mark.parametrize("engine,pair", [(16, p) for p in G.PAIRS16] + [(32, p) for p in G.PAIRS32])
def test_checker_accepts_fp32_results_and_rejects_each_slip(engine, pair):
    """The bound passes an honest fp32 evaluation of the same problem (torch fp32 products and epilogue) and fails each
    wrong reference that applies to the pair: a K tile of 32 dropped, the result doubled (an acc_scale slip), bias
    omitted, alpha or gamma applied twice, the head's re and im swapped."""
    epi, out = pair if engine == 16 else (pair[1], G.OUT_F32)
    pro = pair[0] if engine == 32 else G.PRO_NONE
    p = _problem(epi)
    a = G.elu(p["a"]) if pro == G.PRO_ELU else p["a"]
    acc = a @ p["w"].t()
    mag = a.abs() @ p["w"].abs().t()
    refs, bounds = G.epilogue(epi, out, acc, mag, bias=p["bias"], R=p["R"], gamma=p["gamma"], alpha=p["alpha"],
                              head_kb=p["head_kb"])
    got = _result(p, epi, out, pro, dtype=torch.float32)
    for g, r, b in zip(got, refs, bounds):
        bad, worst, finite = G.check(g, r, b)
        assert finite and bad == 0, (G.EPI_NAMES[epi], worst)
    for slip in _slips(epi):
        wrong = _result(p, epi, out, pro, **{slip: True})
        rejected = [G.check(got_c, w, b)[0] > 0 for got_c, w, b in zip(got, wrong, bounds)]
        # the checker compares the honest result against the wrong reference: every output must expose the slip
        assert all(rejected), (G.EPI_NAMES[epi], G.OUT_NAMES[out], slip)


# ---------------------------------------------------------------------------------------------- refusals
FAKE = 1 << 20          # 256-byte aligned stand-ins for device pointers: a refused descriptor never dereferences them


def _desc(**kw):
    from wavtokenizer_amd import _capi
    d = _capi.WtGemmDesc()
    d.size = ctypes.sizeof(d)
    d.engine, d.epi, d.out, d.pro = 0, G.EPI_BIAS, G.OUT_F32, G.PRO_NONE
    d.M, d.N, d.K = 64, 64, 64
    d.T_in = d.T_out = 64
    d.Cin, d.taps, d.stride, d.dil = 64, 1, 1, 1
    d.nz, d.alpha = 1, 1.0
    d.a_rstride, d.w_rstride, d.c_rstride = 64, 64, 64
    d.A, d.B, d.C, d.bias = FAKE, 2 * FAKE, 3 * FAKE, 4 * FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("what,kw,msg", [
    ("unsupported pair", dict(epi=G.EPI_BIAS_GELU, out=G.OUT_F32), "unsupported epilogue"),
    ("unsupported gemm.hip pair", dict(engine=1, pro=G.PRO_ELU, epi=G.EPI_BIAS_GELU), "unsupported prologue"),
    ("misaligned stride", dict(a_rstride=80, T_in=64), "multiples of 32"),
    ("A2 with taps > 1", dict(A2=5 * FAKE, K1=32, K=128, Cin=64, taps=2, pad_left=1, w_rstride=128), "second K source"),
    ("head without bias", dict(epi=G.EPI_HEAD, out=G.OUT_S32, head_kb=32, bias=None), "head epilogue needs a bias"),
    ("dual output without C2", dict(out=G.OUT_S32_DUAL_ELU), "needs C2"),
    ("F32_AND_S32 without C2", dict(out=G.OUT_F32_AND_S32), "needs C2"),
    ("gamma missing", dict(epi=G.EPI_BIAS_GAMMA_RES, R=6 * FAKE), "gamma"),
    ("descriptor of another size", dict(size=8), "another size"),
])
def test_probe_refuses_before_any_hip_call(what, kw, msg):
    """Descriptors the launchers refuse come back as WT_ERR_INVALID with the launcher's message; the checks run before
    the operands are split, so no device memory is read or written (the pointers here are not even valid)."""
    from wavtokenizer_amd import _capi
    d = _desc(**kw)
    assert _capi.lib.wt_gemm_probe(ctypes.byref(d), None, ctypes.c_void_p(7 * FAKE), None) == -1, what
    assert msg in _capi.lib.wt_last_error().decode(), (what, _capi.lib.wt_last_error())
