"""The fused encoder kernels of one length, one launch at a time through wt_resblock_probe (the plans' own launchers), against
the float64 references of tests/enc_ref.py: resblock16_kernel in its three plain forms and its two DOWN forms, resblock_kernel
(the fp32 chain).  Per case: (a) the launch form the launcher reports is the one the case is named for, with its grid and tile
count; (b) every element within its propagated bound, all finite (gemm_ref.check: no sampling, no element excluded); (c) the
guard words around the NaN-prefilled output untouched; (d) the range status word clear.  The last test compares the
instantiations the session reached with the ones the launchers can pick.  tests/test_enc_checks.py holds the CPU half: the
bounds pass honest fp32 and split-f16 evaluations and reject the slips."""
import ctypes

import pytest
import torch

from tests import enc_ref as E
from tests import gemm_ref as G
from tests import parity_log
from tests.util import synth_state_dict

pytestmark = pytest.mark.gpu

GUARD = 64                       # fp32 words of sentinel before and after every output
SENT = -559038737                # 0xDEADBEEF
NAN_BITS = 0x7FC00000
HIT = set()                      # (kernel, C, fold, down, fpw[, "wrapped"]) reached in this session
WORST = {}                       # family -> worst |got - ref| / bound
T_LIST = [1, 2, 3, 4, 125, 126, 127, 128, 129, 252, 253, 256, 257]      # tile seams at VALID = 126 (fold) and 128
OUT_COMBOS = [(0, 0), (1, 1), (0, 1)]                                    # (elu_out, out_s32)
FORMS = {        # name: (arch, stage, C, fold, frames per wave, frames of y per tile)
    "c32_fold": ("hop600", 1, 32, 1, 32, 126),
    "c32_plain": ("hop600", 1, 32, 0, 32, 128),
    "c64": ("hop600", 4, 64, 0, 16, 128),
}
DOWN = {4: "hop600", 2: "hop320"}


class Out:
    """A device output of n fp32 words between two guard runs, pre-filled with NaN (every logical element must be written)."""

    def __init__(self, n):
        self.n = n
        h = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32)
        h[GUARD:GUARD + n] = NAN_BITS
        self.buf = h.cuda()
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def host(self):
        h = self.buf.cpu()
        assert bool((h[:GUARD] == SENT).all()) and bool((h[GUARD + self.n:] == SENT).all()), "guard words overwritten"
        return h[GUARD:GUARD + self.n]


def ncu():
    from wavtokenizer_amd import _capi
    cu = ctypes.c_int32()
    assert _capi.lib.wt_device_info(torch.cuda.current_device(), ctypes.byref(cu), None, None) == 0
    return cu.value


_WEIGHTS = {}


def weights(arch, stage):
    """(float64 reference weights, device arrays in the kernels' layouts) of encoder resblock `stage`; stage 1 comes with the
    first conv and its stage's down conv."""
    key = (arch, stage)
    if key not in _WEIGHTS:
        W = E.stage_weights(synth_state_dict(arch), stage, down=3 if stage == 1 else None)
        C = W["ws"].shape[0]
        dev = lambda t: t.float().contiguous().cuda()
        D = dict(e0_w=dev(W["e0w"][:, 0, :].t()), e0_b=dev(W["e0b"]), w3=dev(W["w3"].permute(0, 2, 1)), b3=dev(W["b3"]),
                 w1=dev(W["w1"].reshape(C, C // 2)), b1=dev(W["b1"]), ws=dev(W["ws"].reshape(C, C)), bs=dev(W["bs"]))
        if "wd" in W:
            D["wd"], D["bd"] = dev(W["wd"].permute(0, 2, 1)), dev(W["bd"])
        _WEIGHTS[key] = (W, D)
    return _WEIGHTS[key]


def run_rb(D, B, T, C, x=None, wav=None, r=0, elu_out=0, out_s32=0, fp32_chain=0, mix=None):
    """One probe launch: x [B][C][T] / wav [B][T] (host, reference layout) -> (form, output words [B][rows][channels] int32).
    mix: (address of clip 0's length word, of its readable-length word) in a device geometry table."""
    from wavtokenizer_amd import _capi
    d = _capi.WtResblockDesc()
    d.size = ctypes.sizeof(d)
    d.B, d.T, d.C, d.r, d.elu_out, d.out_s32, d.fp32_chain = B, T, C, r, elu_out, out_s32, fp32_chain
    keep = []
    if wav is not None:
        keep.append(wav.float().contiguous().cuda())
        d.wav, d.e0_w, d.e0_b = keep[0].data_ptr(), D["e0_w"].data_ptr(), D["e0_b"].data_ptr()
    else:
        keep.append(x.transpose(1, 2).float().contiguous().cuda())
        d.x = keep[0].data_ptr()
    for n in ("w3", "b3", "w1", "b1", "ws", "bs"):
        setattr(d, n, D[n].data_ptr())
    rows, ch = (-(-T // r), 64) if r else (T, C)
    if r:
        d.wd, d.bd = D["wd"].data_ptr(), D["bd"].data_ptr()
    y = Out(B * rows * ch)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    d.y, d.status = y.ptr, status.data_ptr()
    if mix is not None:
        d.mix_T, d.mix_Tread = mix
    f = _capi.WtResblockForm()
    rc = _capi.lib.wt_resblock_probe(ctypes.byref(d), ctypes.byref(f), None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    assert int(status[0]) == 0, f"range status {int(status[0])} on an in-range problem"
    return f, y.host().reshape(B, rows, ch)


def decode(words, s32):
    """[rows][C] output words -> float64 values."""
    rows, C = words.shape
    if rows == 0:
        return torch.zeros(0, C, dtype=torch.float64)
    if s32:
        return G.decode_s32_rows(words.contiguous().view(torch.int16).reshape(-1), rows, C)
    return words.contiguous().view(torch.float32).double()


def check(got, ref, bound, what, family, worst=WORST):
    nbad, frac, finite = G.check(got, ref, bound)
    print(f"{what}: worst error {frac:.3g} of the bound")
    assert finite, f"{what}: an element was not written or is not finite"
    assert nbad == 0, f"{what}: {nbad} elements outside the bound (worst {frac:.3g} x bound)"
    worst[family] = max(worst.get(family, 0.0), frac)
    return frac


def check_form(f, kernel, C, fold, down, fpw, tiles, hit=HIT):
    """The instantiation, and a grid sized as the launchers size it: one workgroup per tile up to the resident slots."""
    assert (f.kernel, f.C, f.fold, f.down, f.fpw) == (kernel, C, fold, down, fpw), (f.kernel, f.C, f.fold, f.down, f.fpw)
    assert f.tiles == tiles and f.lds > 0 and f.block == (2 * 128 if kernel == 2 and C == 32 else 2 * 64 if kernel == 2 else 128 // fpw * 64)
    slots = ncu() * min(4, 160 * 1024 // f.lds)
    assert f.grid == min(tiles, slots), (f.grid, tiles, slots)
    hit.add((kernel, C, fold, down, fpw))
    if f.grid < f.tiles:
        hit.add((kernel, C, fold, down, fpw, "wrapped"))


def inputs(form, B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    if form == "c32_fold":
        return dict(wav=torch.randn(B, T, generator=gen).float().double())
    return dict(x=torch.randn(B, FORMS[form][2], T, generator=gen).float().double())


def _one_length(form, B, T, combos, seed):
    arch, stage, C, fold, fpw, valid = FORMS[form]
    W, D = weights(arch, stage)
    inp = inputs(form, B, T, seed)
    for elu_out, out_s32 in combos:
        f, words = run_rb(D, B, T, C, elu_out=elu_out, out_s32=out_s32, **inp)
        check_form(f, 0, C, fold, 0, fpw, B * -(-T // valid))
        ref, bound = E.resblock(W, elu_out=elu_out, out_s32=out_s32, **inp)
        check(decode(words.reshape(B * T, C), out_s32).reshape(B, T, C), ref, bound, f"{form} T={T} elu={elu_out} s32={out_s32}",
              f"resblock16 {form}")
    return f


@pytest.mark.parametrize("T", T_LIST)
@pytest.mark.parametrize("form", list(FORMS))
def test_resblock16(form, T):
    _one_length(form, 3, T, OUT_COMBOS, seed=100 * T + len(form))


@pytest.mark.parametrize("form", list(FORMS))
def test_resblock16_wrapped_grid(form):
    """More tiles than resident workgroups: the persistent loop (tile += gridDim.x, the parked prefetch and, with the first
    conv folded in, the double-buffered waveform window) runs, and every seam it crosses is inside the bound."""
    arch, stage, C, fold, fpw, valid = FORMS[form]
    _W, D = weights(arch, stage)
    f0, _ = run_rb(D, 1, 4, C, **inputs(form, 1, 4, 0))
    slots = ncu() * min(4, 160 * 1024 // f0.lds)
    B = 4 if C == 32 else 3
    T = valid * (slots // B + 2) - 5                   # tiles = B * (slots // B + 2) > slots
    f = _one_length(form, B, T, [(1, 1)], seed=7)
    assert f.grid < f.tiles, (f.grid, f.tiles)


def _down_lengths(r):
    opt = (126 - 2 * r) // r + 1
    span = opt * r                                      # samples per output tile: 120 (r = 4), 124 (r = 2)
    exact = span * 9
    return list(range(1024, 1032)) + [exact - 1, exact, exact + 1]


def _down(r, B, T, seed):
    W, D = weights(DOWN[r], 1)
    gen = torch.Generator().manual_seed(seed)
    wav = torch.randn(B, T, generator=gen).float().double()
    f, words = run_rb(D, B, T, 32, wav=wav, r=r)
    opt = (126 - 2 * r) // r + 1
    Td = -(-T // r)
    check_form(f, 0, 32, 1, r, 32, B * -(-Td // opt))
    ref, bound = E.resblock(W, wav=wav, down=r)
    got = decode(words.reshape(B * Td, 64), 0).reshape(B, Td, 64)
    check(got, ref, bound, f"down r={r} T={T}", f"resblock16 down r={r}")
    edge = torch.tensor([0, 1, Td - 2, Td - 1])
    check(got[:, edge], ref[:, edge], bound[:, edge], f"down r={r} T={T} first / last two frames", f"resblock16 down r={r} edge frames")
    return f


@pytest.mark.parametrize("r,T", [(r, T) for r in (4, 2) for T in _down_lengths(r)])
def test_resblock16_down(r, T):
    """Every residue of the stride (the last window completed by extra reflected padding), the shifted last window, an exact
    number of output tiles, one frame more, one less."""
    _down(r, 3, T, seed=7 * T + r)


@pytest.mark.parametrize("r", [4, 2])
def test_resblock16_down_wrapped_grid(r):
    opt = (126 - 2 * r) // r + 1
    _W, D = weights(DOWN[r], 1)
    f0, _ = run_rb(D, 1, 1024, 32, wav=torch.zeros(1, 1024, dtype=torch.float64), r=r)
    slots = ncu() * min(4, 160 * 1024 // f0.lds)
    T = opt * r * (slots // 3 + 2) - 3                 # no multiple of the stride: the last window is shifted and padded
    f = _down(r, 3, T, seed=r)
    assert f.grid < f.tiles, (f.grid, f.tiles)


@pytest.mark.parametrize("T", T_LIST)
@pytest.mark.parametrize("form", list(FORMS))
def test_resblock_fp32_chain(form, T):
    """resblock_kernel (WT_PLAN_FLAG_FP32_GEMM) for every C resblock_fusable accepts, under the exact-product bound."""
    arch, stage, C, fold, _fpw, _valid = FORMS[form]
    W, D = weights(arch, stage)
    inp = inputs(form, 3, T, seed=31 * T + C)
    rows = 128 if C == 32 else 64
    for elu_out in (0, 1):
        f, words = run_rb(D, 3, T, C, elu_out=elu_out, fp32_chain=1, **inp)
        check_form(f, 2, C, fold, 0, 32, 3 * -(-T // rows))
        ref, bound = E.resblock(W, elu_out=elu_out, chain=E.F32, **inp)
        check(decode(words.reshape(3 * T, C), 0).reshape(3, T, C), ref, bound, f"fp32 {form} T={T} elu={elu_out}", f"resblock fp32 {form}")


def test_every_instantiation_was_reached():
    """Runs last: the instantiations the cases above reported are all that launch_resblock16, launch_resblock16_down and
    launch_resblock can pick, each also with a wrapped grid where a case asks for one; the worst fraction of the bound per
    family goes to the parity log (none above 1: the cases assert it)."""
    for fam, w in sorted(WORST.items()):
        parity_log.record(f"encoder_ops {fam}", worst_of_bound=w)
    rb16 = {(0, 32, 1, 0, 32), (0, 32, 0, 0, 32), (0, 64, 0, 0, 16), (0, 32, 1, 4, 32), (0, 32, 1, 2, 32)}
    want = rb16 | {k + ("wrapped",) for k in rb16} | {(2, 32, 1, 0, 32), (2, 32, 0, 0, 32), (2, 64, 0, 0, 32)}
    assert HIT == want, HIT ^ want
