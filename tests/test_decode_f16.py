"""set_gemm_precision("f16") / WT_PLAN_FLAG_F16_GEMM: the decode plans on the one-product GEMM twin.  The mode changes the
decoder's waveform and nothing else; inside the mode every identity of the default mode holds bit for bit (decode from codes,
batch invariance across tile forms, mixed-length batches, graph replay); the flag is refused where it means nothing; and the
waveform sits where the rounding of the GEMM operands to f16 puts it: within a factor 3 of E, the distance of the float64
emulation of tests/f16_ref.py from the plain float64 run of the oracle (computed on the CPU, never from a GPU output)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import f16_ref

# E per fixture: rel-L2 of f16_ref.decode_f64(q=True) from the oracle's float64 decode of the fixture's codes, bandwidth 0
# (test_emulated_error_is_the_recorded_one recomputes both to 1 %; profiles/f16_mode_error.txt has them beside the GPU's figures)
E_EMULATED = {"hop600": 2.937e-3, "hop320": 2.669e-3}
FIXTURE = "b2_t72000"


def _bw(i):
    return torch.tensor([i])


_REF = {}


def _reference(name):
    """(codes [1, B, L] int64, features float64, the oracle's float64 waveform) of the fixture: computed once, shared, never modified."""
    from oracle.cpu_ref import OracleWavTokenizer
    from tests.util import load_case, synth_state_dict
    from wavtokenizer_amd import NAMED_ARCHS
    if name not in _REF:
        sd = synth_state_dict(name)
        sd64 = {k: torch.from_numpy(v).double() if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in sd.items()}
        orc = OracleWavTokenizer(NAMED_ARCHS[name], sd64)
        codes = torch.from_numpy(load_case(name, FIXTURE)["codes"])
        with torch.inference_mode():
            feats = orc.codes_to_features(codes)
            wav = orc.decode(feats, _bw(0))
        assert feats.dtype == torch.float64 and wav.dtype == torch.float64
        _REF[name] = (codes, feats, wav)
    return _REF[name]


@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_emulated_error_is_the_recorded_one(name):
    """CPU: E is what the emulation gives today, and the emulation without the rounding is the oracle's float64 decoder."""
    from tests.util import synth_state_dict
    from wavtokenizer_amd import NAMED_ARCHS
    _codes, feats, wav = _reference(name)
    arch, sd = NAMED_ARCHS[name], synth_state_dict(name)
    with torch.inference_mode():
        plain = f16_ref.decode_f64(arch, sd, feats[:1, :, :40], 0, q=False)
        emu = f16_ref.decode_f64(arch, sd, feats, 0, q=True)
    from oracle.cpu_ref import OracleWavTokenizer
    sd64 = {k: torch.from_numpy(v).double() if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in sd.items()}
    with torch.inference_mode():
        want = OracleWavTokenizer(arch, sd64).decode(feats[:1, :, :40], _bw(0))
    assert f16_ref.rel_l2(plain, want) < 1e-11
    E = f16_ref.rel_l2(emu, wav)
    print(f"{name}: emulated E = {E:.4e} (recorded {E_EMULATED[name]:.4e})")
    assert abs(E - E_EMULATED[name]) <= 0.01 * E_EMULATED[name], (E, E_EMULATED[name])


# ------------------------------------------------------------------------------------------------------ GPU
_MODELS = {}


def _model(name):
    from tests.util import synth_state_dict
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer
    if name not in _MODELS:
        m = WavTokenizer.from_arch(NAMED_ARCHS[name])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(name).items()}, strict=False)
        _MODELS[name] = m.eval().to("cuda")
    return _MODELS[name]


class _f16:
    def __init__(self, m):
        self.m = m

    def __enter__(self):
        self.m.set_gemm_precision("f16")

    def __exit__(self, *a):
        self.m.set_gemm_precision("f16x3")
        self.m.set_graph_max_clips(16)


def _codes(m, B, L, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, m.arch.vq_bins, size=(1, B, L))).cuda()


def _no_status(m):
    m.check_status()
    assert not m.fallback_events


def _f16_plans(m):
    from wavtokenizer_amd import _capi
    return [k for k in m._engine.plans if k[3] & _capi.WT_PLAN_FLAG_F16_GEMM]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_mode_changes_the_decoder_and_nothing_else(name):
    from wavtokenizer_amd import _capi, synth
    m = _model(name)
    with pytest.raises(ValueError):
        m.set_gemm_precision("bf16")
    wav_in = torch.from_numpy(synth.make_clips(2, 12000, seed=3)).cuda()
    feats0, codes0 = m.encode_infer(wav_in, bandwidth_id=_bw(0))
    dflt = m.decode(feats0, bandwidth_id=_bw(0))
    with _f16(m):
        feats1, codes1 = m.encode_infer(wav_in, bandwidth_id=_bw(0))
        assert torch.equal(feats1, feats0) and torch.equal(codes1, codes0)
        assert torch.equal(m.codes_to_features(codes0), feats0)
        got = m.decode(feats0, bandwidth_id=_bw(0))
        assert got.shape == dflt.shape and bool(torch.isfinite(got).all())
        assert not torch.equal(got, dflt)
        # decode from codes is the bits of the composition, in this mode too
        assert torch.equal(m.decode_codes(codes0, bandwidth_id=_bw(0)), got)
        # a clip decoded alone is its slot of a batch (B = 1 and B = 3 run on different tile forms)
        c3 = _codes(m, 3, 33, seed=11)
        f3 = m.codes_to_features(c3)
        w3 = m.decode(f3, bandwidth_id=_bw(1))
        for j in range(3):
            assert torch.equal(m.decode(f3[j:j + 1], bandwidth_id=_bw(1)), w3[j:j + 1]), j
        # only decode kinds carry the flag
        kinds = {k[0] for k in _f16_plans(m)}
        assert kinds and kinds <= {_capi.WT_PLAN_DECODE, _capi.WT_PLAN_DECODE_MIXED, _capi.WT_PLAN_DECODE_CODES, _capi.WT_PLAN_DECODE_CODES_MIXED}
    assert torch.equal(m.decode(feats0, bandwidth_id=_bw(0)), dflt)       # and the default is back
    _no_status(m)


@pytest.mark.gpu
def test_identities_inside_the_mode():
    from wavtokenizer_amd import _capi
    m = _model("hop600")
    with _f16(m):
        # mixed-length batches: each clip the bits of its own call
        clips = [_codes(m, 1, L, seed=L)[:, 0, :] for L in (5, 33, 64)]
        feats = [m.codes_to_features(c)[0] for c in clips]
        solo = [m.decode(f[None], bandwidth_id=_bw(0)) for f in feats]
        many = m.decode_many(feats, bandwidth_id=_bw(0))
        cmany = m.decode_codes_many(clips, bandwidth_id=_bw(0))
        for j in range(3):
            assert torch.equal(many[j], solo[j]), j
            assert torch.equal(cmany[j], solo[j]), j
        mixed = {k[0] for k in _f16_plans(m)} & {_capi.WT_PLAN_DECODE_MIXED, _capi.WT_PLAN_DECODE_CODES_MIXED}
        assert mixed == {_capi.WT_PLAN_DECODE_MIXED, _capi.WT_PLAN_DECODE_CODES_MIXED}      # (the batches were batched)
        # graph replay: the third call in a row is a replay, and the bits of the eager call
        f1 = m.codes_to_features(_codes(m, 1, 33, seed=7))
        for _ in range(3):
            replayed = m.decode(f1, bandwidth_id=_bw(0))
        (key, plan), = [(k, p) for k, (p, _ws) in m._engine.plans.items()
                        if k[0] == _capi.WT_PLAN_DECODE and k[1] == 1 and k[2] == 33 and k[3] & _capi.WT_PLAN_FLAG_F16_GEMM]
        assert key[3] & _capi.WT_PLAN_FLAG_GRAPH and _capi.lib.wt_plan_graph_replays(plan) >= 1
        m.set_graph_max_clips(0)
        eager = m.decode(f1, bandwidth_id=_bw(0))
        assert torch.equal(replayed, eager)
        # the big persistent tile forms: pwconv1 at B = 12, L = 120 is past launch16s_tiled's t128 <= 100 forms
        B, L = 12, 120
        assert ((B * L + 127) // 128) * ((m.arch.intermediate_dim + 127) // 128) > 100
        cb = _codes(m, B, L, seed=5)
        fb = m.codes_to_features(cb)
        wb = m.decode(fb, bandwidth_id=_bw(0))
        assert bool(torch.isfinite(wb).all())
        assert torch.equal(m.decode_codes(cb, bandwidth_id=_bw(0)), wb)
        assert torch.equal(m.decode(fb[4:5], bandwidth_id=_bw(0)), wb[4:5])
    _no_status(m)


@pytest.mark.gpu
def test_c_abi_flag():
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.pretrained import _ptr, _stream_ptr
    m = _model("hop600")
    dev = m._ensure_engine()
    lib = _capi.lib
    F16 = _capi.WT_PLAN_FLAG_F16_GEMM
    assert F16 == 128
    for kind, length in ((_capi.WT_PLAN_ENCODE, 12000), (_capi.WT_PLAN_HEAD, 20), (_capi.WT_PLAN_SEANET_DECODER, 20)):
        p = ctypes.c_void_p()
        assert lib.wt_plan_create(m._engine.model, kind, 1, length, F16, ctypes.byref(p)) == _capi.WT_ERR_INVALID, kind
        assert b"WT_PLAN_FLAG_F16_GEMM" in lib.wt_last_error(), lib.wt_last_error()
    for other in (_capi.WT_PLAN_FLAG_FP32_GEMM, _capi.WT_PLAN_FLAG_UNFUSED):
        p = ctypes.c_void_p()
        assert lib.wt_plan_create(m._engine.model, _capi.WT_PLAN_DECODE, 1, 20, F16 | other, ctypes.byref(p)) == _capi.WT_ERR_INVALID
        assert b"WT_PLAN_FLAG_F16_GEMM" in lib.wt_last_error(), lib.wt_last_error()
    # with one range site on fp32 operands (the per-site range fallback: the first ConvNeXt block, the attention block, the head)
    # the plan runs, and stays inside the bar
    codes, _feats, ref = _reference("hop600")
    feats = m.codes_to_features(codes.cuda())
    B, _, L = feats.shape
    E = E_EMULATED["hop600"]
    for what, site in (("convnext.0", _capi.WT_SITE_CNX0), ("pos_net.2", _capi.WT_SITE_ATTN), ("the head", _capi.WT_SITE_HEAD)):
        plan, ws = m._engine.plan(_capi.WT_PLAN_DECODE, B, L, F16, dev, 1 << site)
        wav = torch.empty((B, m._wave_len(L)), device=dev)
        _capi.check(lib.wt_decode(plan, _ptr(feats), 0, _ptr(wav), _ptr(None), _ptr(ws), _stream_ptr(dev)), "wt_decode")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(wav).all()), what
        err = f16_ref.rel_l2(wav.cpu(), ref)
        print(f"f16 plan with {what} on fp32 operands: rel-L2 {err:.3e} from float64 (E = {E:.3e})")
        assert E / 3 <= err <= 3 * E, (what, err, E)
    # KEEP_STAGES and RANGE_REPORT combine with the flag
    for extra in (_capi.WT_PLAN_FLAG_KEEP_STAGES, _capi.WT_PLAN_FLAG_RANGE_REPORT):
        p = ctypes.c_void_p()
        assert lib.wt_plan_create(m._engine.model, _capi.WT_PLAN_DECODE_CODES, 1, 20, F16 | extra, ctypes.byref(p)) == 0, lib.wt_last_error()
        lib.wt_plan_destroy(p)
    m._engine.drop(lambda k: k[3] & F16)
    _no_status(m)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_waveform_error_against_float64(name):
    """Measured on an MI355X (profiles/f16_mode_error.txt): hop600 2.898e-3 = 0.99 E, hop320 2.751e-3 = 1.03 E; the default mode
    on the same fixtures 3.3e-6 and 3.1e-6."""
    m = _model(name)
    codes, _feats, ref = _reference(name)
    dflt = f16_ref.rel_l2(m.decode_codes(codes.cuda(), bandwidth_id=_bw(0)).cpu(), ref)
    with _f16(m):
        got = m.decode_codes(codes.cuda(), bandwidth_id=_bw(0))
    err = f16_ref.rel_l2(got.cpu(), ref)
    E = E_EMULATED[name]
    print(f"f16_mode_error {name} {FIXTURE}: emulated E {E:.4e}, GPU f16 mode {err:.4e} ({err / E:.2f} E), GPU default {dflt:.4e}")
    assert E / 3 <= err <= 3 * E, (err, E)
    assert dflt <= 1e-4                                        # (the default mode's bar, unchanged)
    _no_status(m)
