"""The SLSTM recurrence kernels alone, through wt_lstm_probe (the function every plan's LSTM step calls), against the float64
reference of tests/lstm_ref.py: lstm_persist_kernel<SMALL> and <BIG>, lstm_step_kernel<true> (split-f16) and <false> (fp32).
Per case: (a) the launch the launchers report: kernel, SMALL exactly when ceil(B / 8) <= 8, clips per XCD, grid, block, dynamic
LDS, number of launches; (b) every element within its bound, propagated through time (gemm_ref.check: no sampling, nothing
excluded); (c) no element of the NaN-prefilled output left unwritten, the guard words around it untouched; (d) status word 0.

Three weight sets are written into the state dict before the model is created, so the three packings of weights.cpp load_lstm
(Wp, W0h / W1h, W0 / W1, b1, the gate-row order) are under test with the kernels: "dense" (the synthetic weights; one and two
steps, where every weight still shows), "contractive" and "few" (few large weights per row; any length: the bound stays flat).
The inputs carry five regimes per hidden unit (lstm_ref.make_inputs).  tests/test_lstm_checks.py is the CPU half: the bound
passes honest fp32 and split-f16 runs on these cases and rejects each slip.

The cases: the persistent kernel by batch shape and over time, both step kernels likewise, elu_out x out_s32 on every kernel
that reaches them, the range report of both implementations, the SEANetDecoder's weight set.  On an MI355X the worst error was
0.49 of the bound (few-large set, every kernel; contractive 0.41, fp32 step kernel 0.29; dense 0.36): where h1 is near 0 the
one rounding of h1 + x is half of the ULP the bound grants it, so a ratio near 0.5 is the most an exact recurrence can show.
Then: a clip's y is bit-equal whatever batch and slot it sits in: within each step kernel, and on the persistent kernel across
its two forms as well (both sum the split-f16 correction products in the same two chains); a NaN in one clip's xg (the default one
and the all-ones pattern, whose f16 image is the persistent exchange's own mark) stays in that clip; which = 1 on a model created
without decoder tensors is refused."""
import ctypes
import math

import pytest
import torch

from tests import gemm_ref as G
from tests import lstm_ref as R
from tests import parity_log

pytestmark = pytest.mark.gpu

H = R.H
GUARD = 64
SENT = -559038737                # 0xDEADBEEF
NAN_BITS = 0x7FC00000
PERSIST, STEP16, STEP32 = 0, 1, 2
KNAME = {PERSIST: "persistent", STEP16: "step split-f16", STEP32: "step fp32"}
LDS_SEEN = {}                   # small -> dynamic LDS bytes the persistent launcher reported
B_FOR_L = {1: 130, 2: 130, 3: 65, 7: 130, 24: 128, 40: 9}      # the largest batch any case runs at each length
WORST = {}


def device_info():
    from wavtokenizer_amd import _capi
    cu, pl = ctypes.c_int32(), ctypes.c_int32()
    assert _capi.lib.wt_device_info(torch.cuda.current_device(), ctypes.byref(cu), None, ctypes.byref(pl)) == 0
    return cu.value, pl.value


def need(kernel):
    if kernel == PERSIST and not device_info()[1]:
        pytest.skip(f"wt_device_info reports no persistent LSTM on this device ({device_info()[0]} compute units)")


# ------------------------------------------------------------------------------------------------ models and references
_MODELS = {}


def model(name):
    """(WavTokenizer, state dict) with weight set `name` as the encoder's SLSTM; "few" is built with a SEANetDecoder whose
    SLSTM holds "few2"."""
    if name not in _MODELS:
        from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer, synth
        from tests.util import manifest
        arch = NAMED_ARCHS["hop600"]
        sd = dict(synth.make_state_dict(arch, seed=manifest()["weight_seed"], with_seanet_decoder=(name == "few")))
        R.put_weights(sd, R.ENC_PREFIX + "13", name)
        if name == "few":
            R.put_weights(sd, R.DEC_PREFIX + "1", "few2")
        m = WavTokenizer.from_arch(arch)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        m = m.eval().to("cuda")
        m._ensure_engine()
        _MODELS[name] = (m, sd)
    return _MODELS[name]


_STATE = {}
_INPUTS = {}


def case_inputs(L):
    if L not in _INPUTS:
        _INPUTS[L] = R.case_inputs(L)
    return _INPUTS[L]


def reference(name, which, B, L, chain, elu_out=0, out_s32=0):
    """(ref, bound) [B][L][H] of the first B clips: the recurrence is computed once per (weights, L, arithmetic) at the largest
    batch of that length and shared, unchanged, by every case."""
    key = (name, which, L, chain.name)
    if key not in _STATE:
        _m, sd = model(name)
        W = R.lstm_weights(sd, R.DEC_PREFIX + "1" if which else R.ENC_PREFIX + "13")
        xg, x = case_inputs(L)
        n = B_FOR_L[L]
        _STATE[key] = R.slstm_state(W, xg[:n], x[:n], chain)
    h1, e_h1 = _STATE[key]
    assert B <= h1.shape[0]
    return R.output_form(h1[:B], e_h1[:B], case_inputs(L)[1][:B], elu_out, out_s32)


# ------------------------------------------------------------------------------------------------ the probe
class Out:
    """n fp32 words between two guard runs, pre-filled with NaN."""

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


def run(name, kernel, xg, x, which=0, elu_out=0, out_s32=0, status_want=0):
    """One probe call on xg [B][L][4][H], x [B][L][H] (host, float64 copies of fp32 values; xg may also be the packed fp32
    [L][B][4 H] itself) -> (form, float64 y [B][L][H], status word)."""
    from wavtokenizer_amd import _capi
    m, _sd = model(name)
    B, L = x.shape[:2]
    packed = xg if xg.dtype == torch.float32 else R.pack_gates(xg.permute(1, 0, 2, 3)).float()
    assert tuple(packed.shape) == (L, B, 4 * H)
    xg_d, x_d = packed.contiguous().cuda(), x.float().contiguous().cuda()
    y = Out(B * L * H)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _capi.WtLstmDesc()
    d.size = ctypes.sizeof(d)
    d.which, d.kernel, d.B, d.L, d.elu_out, d.out_s32 = which, kernel, B, L, elu_out, out_s32
    d.xg, d.x, d.y, d.status = xg_d.data_ptr(), x_d.data_ptr(), y.ptr, status.data_ptr()
    nws = _capi.lib.wt_lstm_probe_workspace_bytes(ctypes.byref(d))
    assert nws > 0, _capi.lib.wt_last_error().decode()
    ws = torch.empty(nws + 256, dtype=torch.uint8, device="cuda")
    wp = (ws.data_ptr() + 255) // 256 * 256
    f = _capi.WtLstmForm()
    rc = _capi.lib.wt_lstm_probe(m._engine.model, ctypes.byref(d), ctypes.byref(f), ctypes.c_void_p(wp), None)
    assert rc == 0, _capi.lib.wt_last_error().decode()
    torch.cuda.synchronize()
    st = int(status[0])
    assert st == status_want, f"status word {st}, expected {status_want}"
    words = y.host()
    if out_s32:
        got = G.decode_s32_rows(words.contiguous().view(torch.int16).reshape(-1), B * L, H).reshape(B, L, H)
    else:
        got = words.view(torch.float32).double().reshape(B, L, H)
    check_form(f, kernel, B, L)
    return f, got, st


def check_form(f, kernel, B, L):
    assert f.kernel == kernel, (f.kernel, kernel)
    if kernel == PERSIST:
        bx = -(-B // 8)
        small = 1 if bx <= 8 else 0
        assert (f.small, f.Bx, f.grid_x, f.grid_y, f.block, f.launches) == (small, bx, 256, 1, 768, 1), \
            (f.small, f.Bx, f.grid_x, f.grid_y, f.block, f.launches)
        # what the launcher asked for fits a CU's 160 KB, is one value per instantiation, and the two instantiations differ
        assert 0 < f.lds <= 160 * 1024, f.lds
        assert LDS_SEEN.setdefault(small, f.lds) == f.lds, (LDS_SEEN, f.lds)
        assert len(set(LDS_SEEN.values())) == len(LDS_SEEN), LDS_SEEN
    else:
        assert (f.small, f.Bx, f.grid_x, f.grid_y, f.block, f.lds, f.launches) == (0, 0, 256, -(-B // 64), 1024, 0, L + 1), \
            (f.small, f.Bx, f.grid_x, f.grid_y, f.block, f.lds, f.launches)


def form_name(kernel, B):
    return KNAME[kernel] + ((" SMALL" if -(-B // 8) <= 8 else " BIG") if kernel == PERSIST else "")


def check(got, ref, bound, what, family):
    nbad, frac, finite = G.check(got, ref, bound)
    print(f"{what}: worst error {frac:.3g} of the bound")
    assert finite, f"{what}: an element was not written or is not finite"
    assert nbad == 0, f"{what}: {nbad} elements outside the bound (worst {frac:.3g} x bound)"
    WORST[family] = max(WORST.get(family, 0.0), frac)
    parity_log.record(f"lstm_ops {family}", worst_of_bound=WORST[family])
    return frac


def one_case(name, kernel, B, L, which=0, elu_out=0, out_s32=0):
    need(kernel)
    xg, x = case_inputs(L)
    _f, got, _st = run(name, kernel, xg[:B], x[:B], which=which, elu_out=elu_out, out_s32=out_s32)
    ref, bound = reference(name, which, B, L, R.F32 if kernel == STEP32 else R.S16, elu_out, out_s32)
    check(got, ref, bound, f"{KNAME[kernel]} {name} B={B} L={L} elu={elu_out} s32={out_s32}", f"{form_name(kernel, B)} {name}")
    return got


# ------------------------------------------------------------------------------------------------ the cases
# SMALL: 1 (seven XCDs idle), 8 (one clip per XCD), 9 (Bx = 2: XCD 4 holds one clip, XCDs 5-7 none), 57 (Bx = 8, the last XCD one
# of eight rows), 64 (full); BIG: 65 (Bx = 9, the last XCD two clips), 100, 128 (16 per XCD, two poll rounds)
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("B", [1, 8, 9, 57, 64, 65, 100, 128])
def test_persistent_batch_shapes(B, L):
    one_case("dense", PERSIST, B, L)


# L = 3 and 7: every exchange buffer rewritten twice; 40 and 24: long runs at small and at full batches
@pytest.mark.parametrize("B,L", [(9, 3), (65, 3), (9, 7), (65, 7), (1, 40), (9, 40), (64, 24), (65, 24), (128, 24)])
@pytest.mark.parametrize("name", ["contractive", "few"])
def test_persistent_over_time(name, B, L):
    one_case(name, PERSIST, B, L)


# three clip tiles at 130, beyond the persistent kernel's limit
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kernel", [STEP16, STEP32])
def test_step_batch_shapes(kernel, B, L):
    one_case("dense", kernel, B, L)


@pytest.mark.parametrize("B,L", [(1, 40), (65, 24), (130, 7)])
@pytest.mark.parametrize("name", ["contractive", "few"])
@pytest.mark.parametrize("kernel", [STEP16, STEP32])
def test_step_over_time(kernel, name, B, L):
    one_case(name, kernel, B, L)


# elu_out x out_s32 on every kernel that reaches them: the fp32 step kernel writes fp32 in every plan (the probe refuses its S32
# form: tests/test_lstm_checks.py)
FORMS = [(k, e, s) for k in (PERSIST, STEP16, STEP32) for e in (0, 1) for s in (0, 1) if not (k == STEP32 and s)]


@pytest.mark.parametrize("B,L", [(9, 7), (65, 3)])
@pytest.mark.parametrize("kernel,elu_out,out_s32", FORMS)
def test_output_forms(kernel, elu_out, out_s32, B, L):
    """The skip input has both signs, so ELU's two sides and its slope term are used."""
    got = one_case("contractive", kernel, B, L, elu_out=elu_out, out_s32=out_s32)
    if elu_out:
        assert bool((got < 0).any()) and bool((got > 0).any()) and float(got.min()) > -1.0


@pytest.mark.parametrize("out_s32", [1, 0])
@pytest.mark.parametrize("kernel", [PERSIST, STEP16])
def test_range_report(kernel, out_s32):
    """One skip value of 7e4 in one clip: as S32 it is beyond the f16 range of the hi half and exactly WT_STATUS_RANGE is
    reported (the persistent kernel tests the value, the step kernel goes through range_report); as fp32 nothing is reported and
    y is finite.  Every other element stays inside its bound either way."""
    from wavtokenizer_amd import _capi
    need(kernel)
    B, L = 9, 7
    xg, x = case_inputs(L)
    xg, x = xg[:B], x[:B].clone()
    x[4, 3, 100] = 7.0e4
    _f, got, _st = run("few", kernel, xg, x, out_s32=out_s32, status_want=_capi.WT_STATUS_BIT_RANGE if out_s32 else 0)
    reference("few", 0, B, L, R.S16)
    h1, e_h1 = _STATE[("few", 0, L, R.S16.name)]
    ref, bound = R.output_form(h1[:B], e_h1[:B], x, 0, out_s32)
    if out_s32:
        assert not math.isfinite(float(got[4, 3, 100]))
        got[4, 3, 100] = ref[4, 3, 100]
    else:
        assert abs(float(got[4, 3, 100]) - 7.0e4) < 1.0
    check(got, ref, bound, f"{KNAME[kernel]} range s32={out_s32}", f"{form_name(kernel, B)} few")


@pytest.mark.parametrize("kernel", [PERSIST, STEP16, STEP32])
def test_seanet_decoder_weights(kernel):
    """which = 1: the SEANetDecoder's SLSTM, which holds another few-large set than the encoder's: a probe that took the wrong
    LstmW would be far outside."""
    one_case("few", kernel, 9, 7, which=1)


def test_model_without_seanet_decoder_is_refused():
    """which = 1 on a model whose state dict holds no SEANetDecoder.  The WavTokenizer class always has the module, so the model
    is created from a state dict without its tensors; the descriptor names real device arrays."""
    from wavtokenizer_amd import NAMED_ARCHS, _capi
    from wavtokenizer_amd.pretrained import _Engine
    m, _sd = model("contractive")
    state = {k: v for k, v in m.state_dict().items() if not k.startswith(R.DEC_PREFIX)}
    assert len(state) < len(m.state_dict())
    eng = _Engine()
    eng.load(NAMED_ARCHS["hop600"], state, torch.cuda.current_device())
    try:
        B, L = 9, 7
        xg = torch.zeros(L, B, 4 * H, device="cuda")
        x = torch.zeros(B, L, H, device="cuda")
        y = torch.zeros(B, L, H, device="cuda")
        ws = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
        for kernel in (PERSIST, STEP16, STEP32):
            d = _capi.WtLstmDesc()
            d.size = ctypes.sizeof(d)
            d.which, d.kernel, d.B, d.L, d.xg, d.x, d.y = 1, kernel, B, L, xg.data_ptr(), x.data_ptr(), y.data_ptr()
            assert _capi.lib.wt_lstm_probe_workspace_bytes(ctypes.byref(d)) <= ws.numel() and ws.data_ptr() % 256 == 0
            assert _capi.lib.wt_lstm_probe(eng.model, ctypes.byref(d), None, ctypes.c_void_p(ws.data_ptr()), None) == _capi.WT_ERR_INVALID
            assert "no SEANetDecoder" in _capi.lib.wt_last_error().decode()
        torch.cuda.synchronize()
        assert float(y.abs().max()) == 0.0
    finally:
        eng.close()


# the first four keep the ids they had before the length became a parameter
@pytest.mark.parametrize("kernel,batches,L,name", [
    pytest.param(PERSIST, (3, 8, 57), 7, "few", id="0-batches0"), pytest.param(PERSIST, (65, 128), 7, "few", id="0-batches1"),
    pytest.param(STEP16, (1, 65, 130), 7, "few", id="1-batches2"), pytest.param(STEP32, (1, 65, 130), 7, "few", id="2-batches3"),
    # across the SMALL / BIG boundary of the persistent kernel (B <= 64 / above).  On the dense weight set: the two forms differed
    # in the order in which they summed the split-f16 correction products, and a row of few large weights has too few of them
    # for the order to show (on that set the forms agreed before they summed alike)
    pytest.param(PERSIST, (8, 65), 7, "dense", id="persistent-8-65-L7"),
    pytest.param(PERSIST, (3, 57, 100, 128), 7, "dense", id="persistent-3-57-100-128-L7"),
    pytest.param(PERSIST, (8, 65), 24, "dense", id="persistent-8-65-L24"),
    pytest.param(PERSIST, (3, 57, 100, 128), 24, "dense", id="persistent-3-57-100-128-L24")])
def test_clip_independence(kernel, batches, L, name):
    """A clip's y is bit-equal whatever batch it sits in and at whatever slot: each batch holds the clips of the smallest
    one, rotated to other rows (and XCDs or clip tiles), among other clips.  Within each step kernel (they sum K across 16
    waves and are not compared with the persistent kernel), and on the persistent kernel across its SMALL and BIG forms too."""
    need(kernel)
    xg, x = case_inputs(L)
    n = batches[0]
    base = None
    equal = True
    for k, B in enumerate(batches):
        shift = 0 if k == 0 else (5 * k) % B
        idx = (torch.arange(B) - shift) % B                 # slot s holds clip idx[s]: clip c sits in slot (c + shift) % B
        _f, got, _st = run(name, kernel, xg[idx], x[idx])
        mine = got[(torch.arange(n) + shift) % B]
        if base is None:
            base = mine
        else:
            same = torch.equal(mine, base)
            equal = equal and same
            assert same, f"{form_name(kernel, B)}: clips differ between B={n} and B={B} by up to {float((mine - base).abs().max()):.3g}"
    parity_log.record(f"lstm_ops clip independence {form_name(kernel, batches[0])} {batches}" + (f" L={L}" if L != 7 else ""), bit_equal=equal)


@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFFFFFFFF])
@pytest.mark.parametrize("kernel", [PERSIST, STEP16, STEP32])
def test_nan_stays_in_its_clip(kernel, pattern):
    """One clip's xg at one step is NaN: the default quiet NaN, and the all-ones pattern, whose f16 image 0xFFFF is the
    persistent exchange's "not written" mark (lstm_persist.hip no_mark stores the canonical NaN instead; a state half left as the
    mark would end in a bounded spin and WT_STATUS_LSTM, which run() would report as a failed assertion).  Status 0, every
    other clip inside its bound, the clip itself inside it before that step and NaN from it on."""
    need(kernel)
    B, L, clip, t_nan = 9, 7, 4, 2
    xg, x = case_inputs(L)
    packed = R.pack_gates(xg[:B].permute(1, 0, 2, 3)).float().contiguous()
    packed.view(torch.int32)[t_nan, clip, :] = pattern - (1 << 32) if pattern >= 1 << 31 else pattern
    assert bool(torch.isnan(packed[t_nan, clip]).all())
    _f, got, _st = run("few", kernel, packed, x[:B])
    ref, bound = reference("few", 0, B, L, R.F32 if kernel == STEP32 else R.S16)
    others = [c for c in range(B) if c != clip]
    check(got[others], ref[others], bound[others], f"{KNAME[kernel]} NaN {pattern:#x}: other clips", f"{form_name(kernel, B)} few")
    check(got[clip, :t_nan], ref[clip, :t_nan], bound[clip, :t_nan], f"{KNAME[kernel]} NaN {pattern:#x}: the clip before it", f"{form_name(kernel, B)} few")
    assert bool(torch.isnan(got[clip, t_nan:]).all()), "the poisoned clip's later outputs are not all NaN"
