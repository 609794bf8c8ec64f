"""Every range site of the decode plan (model.h Site) on fp32 operands: alone, in adjacent pairs (both sides of a shared buffer)
and all together, against the float64 oracle and the fp32 oracle's stage taps; an overflow injected inside a site is answered
by that site alone; and the other plan kinds, flags and many-clip calls that take a site mask.  tests/range_ref.py holds the
masks, the dead-channel edits and the references."""
import ctypes

import numpy as np
import pytest
import torch

from tests import range_ref
from tests.range_ref import BW
from tests.util import rel_l2, synth_state_dict

STAGE_TOL = 3e-5        # test_b2_stage_checkpoints' bar for a stage against the oracle's tap
EDITS = ["embed", "res0", "attn", "res3", "cnx0", "cnx11", "head"]      # range_ref.dead_channel_edits(hop600)
STAGES = ["bb.embed", "bb.pos_net.0", "bb.pos_net.1", "bb.pos_net.2", "bb.pos_net.3", "bb.pos_net.4", "bb.norm"]


# ---------------------------------------------------------------------------------------------------- CPU: the edits
def test_dead_channel_edits_are_sound():
    """Each edit leaves the model as well-conditioned as it was: the fp32 oracle's distance from the float64 oracle with the
    edited weights stays within 2x its distance with the unedited ones on the same features."""
    from wavtokenizer_amd import NAMED_ARCHS
    name = "hop600"
    base = range_ref.reference(name, 2, 50)
    assert EDITS == range_ref.dead_channel_edits(NAMED_ARCHS[name])
    for label in EDITS:
        site, _sd, _feats, ref = range_ref.edited(name, label)
        print(f"dead channel {label} (site {site}): fp32 oracle {ref['e_cpu']:.3e} from float64, unedited {base['e_cpu']:.3e}")
        assert ref["e_cpu"] <= 2.0 * base["e_cpu"], (label, ref["e_cpu"], base["e_cpu"])


# ------------------------------------------------------------------------------------------------------- GPU helpers
_MODELS = {}


def _fresh(name, sd=None):
    from wavtokenizer_amd import NAMED_ARCHS, WavTokenizer
    m = WavTokenizer.from_arch(NAMED_ARCHS[name])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in (sd or synth_state_dict(name)).items()}, strict=False)
    return m.eval().to("cuda")


def _model(name):
    """One model per architecture for parts 1 and 3 (the plans are driven through m._engine.plan; no call changes its state)."""
    if name not in _MODELS:
        _MODELS[name] = _fresh(name)
        _MODELS[name]._ensure_engine()
    return _MODELS[name]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _step_names(plan):
    from wavtokenizer_amd import _capi
    out = []
    for i in range(_capi.lib.wt_plan_num_steps(plan)):
        s = ctypes.c_char_p()
        assert _capi.lib.wt_plan_step_name(plan, i, ctypes.byref(s)) == 0
        out.append(s.value.decode())
    return out


def _buffers(plan):
    """{name: (offset in bytes, elements, format)} of every buffer of the plan."""
    from wavtokenizer_amd import _capi
    lib, out, i = _capi.lib, {}, 0
    while True:
        s = ctypes.c_char_p()
        if lib.wt_plan_buffer_name(plan, i, ctypes.byref(s)) != 0:
            return out
        off, n, fmt = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
        assert lib.wt_plan_buffer_info(plan, s.value, ctypes.byref(off), ctypes.byref(n), ctypes.byref(fmt)) == 0
        out[s.value.decode()] = (off.value, n.value, fmt.value)
        i += 1


def _stage(bufs, ws, name):
    """A kept stage of the workspace as fp32 (an S32 buffer decoded: groups of [32 hi | 32 lo] halves), on the CPU."""
    from wavtokenizer_amd import _capi
    off, n, fmt = bufs[name]
    assert not fmt & _capi.BUF_ELU, name
    raw = ws[off: off + 4 * n]
    if fmt & _capi.BUF_S32:
        h = raw.view(torch.float16).view(-1, 2, 32).float()
        return (h[:, 0, :] + h[:, 1, :] / 2048.0).reshape(-1).cpu()
    return raw.view(torch.float32).cpu()


class _Run:
    """One WT_PLAN_DECODE plan with WT_PLAN_FLAG_KEEP_STAGES (| flags) and a site mask, run once on the features."""

    def __init__(self, m, feats, flags=0, sites=0):
        from wavtokenizer_amd import _capi
        from wavtokenizer_amd.pretrained import _ptr, _stream_ptr
        dev = _dev()
        B, _, L = feats.shape
        self.key = (B, L, flags | _capi.WT_PLAN_FLAG_KEEP_STAGES, sites)
        plan, ws = m._engine.plan(_capi.WT_PLAN_DECODE, B, L, self.key[2], dev, sites)
        self.wav = torch.empty((B, m._wave_len(L)), device=dev)
        self.aux = torch.empty((B, L, m.arch.dim), device=dev)      # the backbone output as the caller gets it: fp32 in every plan
        _capi.check(_capi.lib.wt_decode(plan, _ptr(feats), 0, _ptr(self.wav), _ptr(self.aux), _ptr(ws), _stream_ptr(dev)), "wt_decode")
        torch.cuda.synchronize()
        self.steps = _step_names(plan)
        self.bufs = _buffers(plan)
        self.ws = ws

    def stage_errors(self, arch, taps, B, L):
        """[(stage, rel-L2 from the fp32 oracle's tap)] in plan order."""
        n = arch.num_layers
        names = STAGES + ["bb.convnext.%d" % i for i in (0, n // 2 - 1, n - 1)] + ["bb.out"]
        out = []
        for st in names:
            mine = _stage(self.bufs, self.ws, st).view(B, L, arch.dim)
            ref = taps[st] if st == "bb.out" else taps[st].permute(0, 2, 1)       # the reference is (B, C, T) up to bb.out
            out.append((st, rel_l2(mine.numpy(), ref.numpy())))
        out.append(("the caller's backbone output", rel_l2(self.aux.cpu().numpy(), taps["bb.out"].numpy())))
        return out


def _drop(m, run):
    """Forgets the run's plan (the engine keeps at most 64) once everything has been read from it."""
    from wavtokenizer_amd import _capi
    B, L, flags, sites = run.key
    m._engine.drop(lambda k: k[0] == _capi.WT_PLAN_DECODE and k[1:4] == (B, L, flags) and (k[5] if len(k) > 5 else 0) == sites)


def _expected_formats(arch, default, mask):
    """The formats wt_plan_buffer_info must report under a site mask, from the default plan's: fp32 for the buffers a site in
    the mask owns, the default's for every other one.  bb.h1 and bb.cnx.norm / bb.cnx.mid are shared by the ResNet blocks and
    the ConvNeXt blocks and change format from site to site while the plan is built; the plan reports what its last user left."""
    from wavtokenizer_amd import _capi as c
    want = {k: v[2] for k, v in default.items()}
    owned = {c.WT_SITE_BB_EMBED: ["bb.in"], c.WT_SITE_ATTN: ["bb.attn.qk", "bb.attn.vt", "bb.attn.o"], c.WT_SITE_RES3: ["bb.h1"],
             c.WT_SITE_CNX0 + arch.num_layers - 1: ["bb.cnx.norm", "bb.cnx.mid"], c.WT_SITE_HEAD: ["bb.out", "head.spec"]}
    for names in owned.values():
        for n in names:
            assert want[n] == c.BUF_S32, n                   # (S32 on the default plan: the switch is visible)
    for site, names in owned.items():
        if mask >> site & 1:
            for n in names:
                want[n] = 0
    if mask >> c.WT_SITE_ATTN & 1:
        assert want.pop("bb.attn.p") == c.BUF_S32            # softmax in place: no probabilities buffer
    return want


def _default_core(steps):
    """A kept plan's step names as the default plan's (test_b2_stage_checkpoints): without the residual snapshots, and the row
    pass that the kept plan calls bb.x2 and copies into bb.norm under the name the default plan gives the pass itself."""
    core = [n for n in steps if not n.startswith(("bb.embed", "bb.pos_net.", "bb.convnext."))]
    core = [n for i, n in enumerate(core) if not (n == "bb.norm" and i and core[i - 1] == "bb.x2")]
    return ["bb.norm" if n == "bb.x2" else n for n in core]


def _check_masks(name, B, L, masks):
    """Part 1 for one shape: returns (failures, [(label, rel-L2 from float64)])."""
    from wavtokenizer_amd import NAMED_ARCHS, _capi
    arch, m = NAMED_ARCHS[name], _model(name)
    ref = range_ref.reference(name, B, L)
    feats = range_ref.features(B, L).cuda()
    plain, _ws = m._engine.plan(_capi.WT_PLAN_DECODE, B, L, 0, _dev())
    plain_steps = _step_names(plain)
    base = _Run(m, feats)
    assert _default_core(base.steps) == plain_steps
    range_ref.float64_bars(base.wav.cpu(), ref, f"{name} ({B}, {L}) default")
    fails, errs = [], []
    for label, mask in masks:
        run = _Run(m, feats, sites=mask)
        what = f"{name} ({B}, {L}) {label}"
        try:
            assert bool(torch.isfinite(run.wav).all()), "not finite"
            # the bit took effect: formats, no attn.p under ATTN, other bits than the default plan's, the same steps
            assert {k: v[2] for k, v in run.bufs.items()} == _expected_formats(arch, base.bufs, mask), "buffer formats"
            assert not torch.equal(run.wav, base.wav), "the default plan's bits"
            # (a step without a name of its own carries its last buffer's: softmax in place is "bb.attn.s", not "bb.attn.p")
            attn = bool(mask >> _capi.WT_SITE_ATTN & 1)
            assert ("bb.attn.p" in run.steps) == (not attn) and run.steps.count("bb.attn.s") == int(attn), "softmax step"
            steps = ["bb.attn.p" if n == "bb.attn.s" else n for n in run.steps]
            assert steps == base.steps and _default_core(steps) == plain_steps, "step names"
            stages = run.stage_errors(arch, ref["taps"], B, L)
            bad = [s for s in stages if not s[1] <= STAGE_TOL]
            assert not bad, "first diverging stage %s (rel-L2 %.3g); all: %s" % (*bad[0], stages)
            errs.append((label, range_ref.float64_bars(run.wav.cpu(), ref, what)))
        except AssertionError as e:
            fails.append(f"{what}: {e}")
        _drop(m, run)
    _drop(m, base)
    m.check_status()
    assert not m.fallback_events
    return fails, errs


# ---------------------------------------------------------------------------- 1. every site forced, alone and in pairs
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_every_site_alone_in_adjacent_pairs_and_all_together(name):
    """(2, 50): every mask of range_ref.site_masks.  The waveform meets the float64 bars of the shipped path, every kept stage
    the fp32 oracle's tap, and the plan shows the switch (formats, steps, bits)."""
    from tests import parity_log
    from wavtokenizer_amd import NAMED_ARCHS
    masks = range_ref.site_masks(NAMED_ARCHS[name])
    assert len(masks) == 2 * (7 + NAMED_ARCHS[name].num_layers)
    fails, errs = _check_masks(name, 2, 50, masks)
    if errs:
        worst = max((e for e in errs if e[0] != "all"), key=lambda e: e[1], default=errs[0])
        parity_log.record(f"range_sites[{name}]", worst_site=worst[0], worst_rel_l2=worst[1], masks=len(errs),
                          all_sites_rel_l2=dict(errs).get("all"),
                          cpu_fp32_oracle_rel_l2=range_ref.reference(name, 2, 50)["e_cpu"])
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", [(3, 130), (1, 1)])
@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_sites_across_the_launch_forms(name, B, L):
    """(3, 130): past the 128-frame launch forms of GroupNorm and softmax, Lp = 160 with 30 pad columns in bb.attn.vt and the
    scores; (1, 1): the smallest plan.  The attention block, one ResNet block, the first ConvNeXt block and the head."""
    from wavtokenizer_amd import _capi as c
    masks = [(n, 1 << s) for s, n in ((c.WT_SITE_ATTN, "attn"), (c.WT_SITE_RES1, "res1"), (c.WT_SITE_CNX0, "cnx0"), (c.WT_SITE_HEAD, "head"))]
    fails, _errs = _check_masks(name, B, L, masks)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hop600", "hop320"])
def test_all_sites_is_the_fp32_gemm_plan(name):
    """With every decoder site on fp32 operands build_decode launches the kernels of a WT_PLAN_FLAG_FP32_GEMM plan on the same
    formats: the same bits, in the waveform and in every kept stage."""
    from wavtokenizer_amd import NAMED_ARCHS, _capi
    arch, m = NAMED_ARCHS[name], _model(name)
    B, L = 2, 50
    feats = range_ref.features(B, L).cuda()
    sites = _Run(m, feats, sites=range_ref.all_decoder_sites(arch))
    flag = _Run(m, feats, flags=_capi.WT_PLAN_FLAG_FP32_GEMM)
    assert sites.steps == flag.steps
    assert {k: v[1:] for k, v in sites.bufs.items()} == {k: v[1:] for k, v in flag.bufs.items()}
    assert all(v[2] == 0 for v in flag.bufs.values())
    n = arch.num_layers
    for st in STAGES + ["bb.convnext.%d" % i for i in (0, n // 2 - 1, n - 1)] + ["bb.out"]:
        assert torch.equal(_stage(sites.bufs, sites.ws, st), _stage(flag.bufs, flag.ws, st)), st
    assert torch.equal(sites.wav, flag.wav) and torch.equal(sites.aux, flag.aux)
    _drop(m, sites)
    _drop(m, flag)
    m.check_status()


# ------------------------------------------------------ 2. an overflow inside a site is attributed to that site alone
@pytest.mark.gpu
@pytest.mark.parametrize("label", EDITS)
def test_overflow_inside_a_site_moves_that_site_alone(label):
    """Strict status: the failing call is repeated with the reporting site on fp32 operands and comes back correct."""
    from wavtokenizer_amd import _capi
    name = "hop600"
    site, sd, feats, ref = range_ref.edited(name, label)
    m = _fresh(name, sd)
    m.set_strict_status(True)
    out = m.decode(feats.cuda(), bandwidth_id=BW)
    assert bool(torch.isfinite(out).all())
    assert m._fp32_sites == 1 << site, (bin(m._fp32_sites), site)
    assert not m._plan_flags & _capi.WT_PLAN_FLAG_FP32_GEMM
    range_ref.float64_bars(out.cpu(), ref, f"overflow inside {label}")
    with pytest.raises(_capi.WavTokError, match="fallback"):
        m.check_status()
    m.check_status()


@pytest.mark.gpu
def test_overflow_inside_the_attention_block_asynchronously():
    """Without strict status and without graphs: the first call is poisoned and names the attention block and no site before
    it; the next call runs with that site on fp32 operands."""
    from wavtokenizer_amd import _capi
    name = "hop600"
    site, sd, feats, ref = range_ref.edited(name, "attn")
    assert site == _capi.WT_SITE_ATTN
    m = _fresh(name, sd)
    m.set_strict_status(False)
    m.set_graph_max_clips(0)
    out = m.decode(feats.cuda(), bandwidth_id=BW)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    plan = next(p for k, (p, _w) in m._engine.plans.items() if k[0] == _capi.WT_PLAN_DECODE)
    sites = ctypes.c_uint64()
    _capi.check(_capi.lib.wt_plan_range_sites(plan, ctypes.byref(sites), 0), "wt_plan_range_sites")
    assert sites.value & (1 << site) and not sites.value & ((1 << site) - 1), hex(sites.value)
    out2 = m.decode(feats.cuda(), bandwidth_id=BW)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out2).all())
    assert m._fp32_sites == 1 << site and not m._plan_flags & _capi.WT_PLAN_FLAG_FP32_GEMM
    range_ref.float64_bars(out2.cpu(), ref, "overflow inside attn, the call after")
    with pytest.raises(_capi.WavTokError, match="fallback"):
        m.check_status()


# ------------------------------------------------------------- 3. the other plan kinds and calls that take a site mask
@pytest.mark.gpu
def test_head_plan_with_the_head_site():
    """WT_PLAN_HEAD is the HEAD site as a whole: its bit gives the bits of WT_PLAN_FLAG_FP32_GEMM on the kind, inside the
    float64 bars against the oracle's head."""
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.pretrained import _ptr, _stream_ptr
    name = "hop600"
    m, dev = _model(name), _dev()
    o32, o64 = range_ref.oracles(name, synth_state_dict(name))
    B, L = 2, 50
    with torch.inference_mode():
        x = o32.backbone(range_ref.features(B, L), BW).contiguous()
        w64 = o64.head(x.double())
        ref = {"w64": w64.numpy(), "e_cpu": rel_l2(o32.head(x).numpy(), w64.numpy())}
    xg = x.cuda()
    wavs = {}
    for what, flags, sites in (("default", 0, 0), ("site", 0, 1 << _capi.WT_SITE_HEAD), ("flag", _capi.WT_PLAN_FLAG_FP32_GEMM, 0)):
        plan, ws = m._engine.plan(_capi.WT_PLAN_HEAD, B, L, flags, dev, sites)
        wavs[what] = torch.empty((B, m._wave_len(L)), device=dev)
        _capi.check(_capi.lib.wt_head(plan, _ptr(xg), _ptr(wavs[what]), _ptr(ws), _stream_ptr(dev)), "wt_head")
        torch.cuda.synchronize()
        assert _buffers(plan)["head.in"][2] == (0 if what != "default" else _capi.BUF_S32)
        range_ref.float64_bars(wavs[what].cpu(), ref, f"head plan, {what}")
    assert torch.equal(wavs["site"], wavs["flag"]) and not torch.equal(wavs["site"], wavs["default"])
    m.check_status()


@pytest.mark.gpu
def test_mixed_length_kinds_refuse_every_site():
    from wavtokenizer_amd import NAMED_ARCHS, _capi
    m = _model("hop600")
    for kind in (_capi.WT_PLAN_DECODE_MIXED, _capi.WT_PLAN_DECODE_CODES_MIXED):
        for site, label in range_ref.decoder_sites(NAMED_ARCHS["hop600"]):
            p = ctypes.c_void_p()
            assert _capi.lib.wt_plan_create_ex(m._engine.model, kind, 2, 40, 0, 1 << site, ctypes.byref(p)) == _capi.WT_ERR_INVALID, (kind, label)
            assert b"mixed-length plans run only" in _capi.lib.wt_last_error(), (kind, label)
            assert not p.value
        p = ctypes.c_void_p()
        assert _capi.lib.wt_plan_create_ex(m._engine.model, kind, 2, 40, 0, 0, ctypes.byref(p)) == 0      # (the mask is what it refuses)
        _capi.lib.wt_plan_destroy(p)


@pytest.mark.gpu
def test_many_clip_calls_with_a_site_on_fp32_go_clip_by_clip():
    """A decoder site on fp32 operands takes the decoder off its mixed route: decode_many, decode_codes_many and
    decode_pcm_many return the bits of the per-clip calls on the same model, and make no mixed-length plan."""
    from wavtokenizer_amd import _capi
    m = _fresh("hop600")
    m._fp32_sites = 1 << _capi.WT_SITE_RES1
    rng = np.random.default_rng(17)
    clips = [torch.from_numpy(rng.integers(0, m.arch.vq_bins, size=(1, L))).cuda() for L in (17, 50, 33)]
    feats = [m.codes_to_features(c)[0] for c in clips]
    solo = [m.decode(f[None], bandwidth_id=BW) for f in feats]
    shipped = _model("hop600").decode(feats[1][None], bandwidth_id=BW)
    assert not torch.equal(solo[1], shipped)                                  # (the site is in force)
    for j, w in enumerate(m.decode_many(feats, bandwidth_id=BW)):
        assert torch.equal(w, solo[j]), j
    for j, w in enumerate(m.decode_codes_many(clips, bandwidth_id=BW)):
        assert torch.equal(w, m.decode_codes(clips[j], bandwidth_id=BW)) and torch.equal(w, solo[j]), j
    for j, w in enumerate(m.decode_pcm_many(clips, sample_rates=16000, bandwidth_id=BW)):
        assert torch.equal(w, m.decode_pcm(clips[j], sample_rate=16000, bandwidth_id=BW)[0]), j
    kinds = {k[0] for k in m._engine.plans}
    assert kinds and not kinds & {_capi.WT_PLAN_DECODE_MIXED, _capi.WT_PLAN_DECODE_CODES_MIXED}
    assert all(len(k) > 5 and k[5] == 1 << _capi.WT_SITE_RES1 for k in m._engine.plans)
    m.check_status()
    assert not m.fallback_events and m._fp32_sites == 1 << _capi.WT_SITE_RES1
