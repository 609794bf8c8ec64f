"""GPU: the plan layer's wiring at architectures other than the two the reference ships YAMLs for.

wt_model_create takes dim 256 .. 1024, any intermediate_dim % 32, depths to 32, any codebook size % 4, any four ratios to 16 and
any n_fft that is an even multiple of hop_length; every other end-to-end test runs hop600 or hop320 (dim 768, intermediate_dim 2304,
four AdaLN rows, 4096 codes, n_fft = 4 hop_length, first encoder ratio 4 or 2).  The four variants of tests/golden/arch_*.npz
(written from the real reference by tests/golden/make_golden_archs.py) take the shape-dependent decisions of the plans where
those two never go:
  narrow  ratios (5,4,4,3), 256 / 96 / 1 layer / 1 AdaLN row, 8 codes, n_fft = 2 hop: no fused stage-1 down kernel at any T,
          K/32 = 3 on pwconv2, N = 96, a codebook narrower than one argmax tile, R = 2, rownorm<1>
  mid16   ratios (16,3,2,5), 512 / 1504 / 3 / 4, 1024 codes, n_fft = 6 hop: a down conv with k = 32, the most taps a GEMM gathers
          (ratios above 16 are refused at load: tests/test_arch_variants_host.py), first encoder ratio 5, K/32 = 47 (odd),
          vq_bins no multiple of 192, R = 6, Kq = 736, rownorm<2>
  last16  ratios (5,3,4,16), narrow's other sizes: the largest ratio as the FIRST encoder stage, whose down conv (32 -> 64
          channels, 32 taps) is a GEMM with N = 64: past 19 taps the 256-row tile has no room for its offset tables
  wide    ratios (8,5,4,2), 1024 / 2080 / 2 / 3, 16384 codes: rownorm<4>, GroupNorm group width 32, N = 2080 (no multiple of
          128 or 192), 85.3 argmax tiles, three AdaLN rows
each on `small` (B = 2, 6 frames with a ragged last hop: the small-problem GEMM forms alone) and `rows` (B = 8, L = 130: across
128, 1040 GEMM rows: the 128-row tile forms).  No frame of a fixture has a float64 top-2 margin under NEAR_TIE_MARGIN, so no
code mismatch is excused anywhere in this file.
"""
import numpy as np
import pytest
import torch

from tests import arch_ref as A
from tests.test_gpu_parity import FUSED_AWAY, STAGE_TOL
from tests.util import WAV_REL_TOL, check_codes, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=A.VARIANTS)
def vm(request):
    from wavtokenizer_amd import WavTokenizer
    name = request.param
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    m = WavTokenizer.from_arch(A.variant(name)[0])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in A.state_dict(name).items()}, strict=False)
    return name, m.eval().to("cuda")


def _bw(name, case):
    return torch.tensor([A.variant(name)[1][case][3]])


def _check_waveform(name, case, out, what):
    """The waveform against the fixture: whole clips where the fixture holds them (`rows`: clip 0), every clip's norm."""
    g = A.variant(name)[2]
    want = g[f"{case}/wav_out"]
    assert out.shape[1] == want.shape[1], (what, out.shape, want.shape)
    err = rel_l2(out[:want.shape[0]], want)
    assert err < WAV_REL_TOL, (what, err)
    l2, want_l2 = np.sqrt((out.astype(np.float64) ** 2).sum(axis=1)), g[f"{case}/wav_out_l2"]
    assert l2.shape == want_l2.shape and (np.abs(l2 - want_l2) < WAV_REL_TOL * want_l2).all(), (what, l2, want_l2)
    return err


@pytest.mark.parametrize("path", ["shipped", "unfused"])
@pytest.mark.parametrize("case", A.CASES)
def test_stage_taps(vm, case, path):
    """tests/test_gpu_parity.py test_b2_stage_checkpoints on the variants.  shipped: every tap the default plan's kernels keep
    (WT_PLAN_FLAG_KEEP_STAGES only un-aliases their buffers) against the oracle's whole tensor and the fixture's head;
    unfused: the debug twin's raw fp32 tensors against the fixture's l2 and head.  Then the codes and the waveform."""
    import torch.nn.functional as F
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd._capi import WavTokError
    from tests import parity_log
    name, m = vm
    arch, cases, g = A.variant(name)
    B, T, _seed, _ = cases[case]
    bw = _bw(name, case)
    L = arch.frames(T)
    H = int(g["head_steps"])
    wav = torch.from_numpy(A.clips(name, case)).cuda()
    orc = A.oracle_run(name, case)
    assert torch.equal(orc["codes"], torch.from_numpy(g[f"{case}/codes"]))          # the oracle is the fixture's source
    m.set_debug_keep_stages(True, unfused=(path == "unfused"))
    try:
        feats, codes = m.encode_infer(wav, bandwidth_id=bw)
        out = m.decode(feats, bandwidth_id=bw)
        torch.cuda.synchronize()
        report, skipped = [], set()
        stages = [k.split("/")[2] for k in g.files if k.startswith(f"{case}/tap/") and k.endswith("/l2")]
        for st in stages:
            shape = tuple(int(v) for v in g[f"{case}/tap/{st}/shape"])
            kind, length = (_capi.WT_PLAN_ENCODE, T) if st.startswith("enc.") else (_capi.WT_PLAN_DECODE, L)
            try:
                buf, fmt = m.debug_stage(kind, B, length, st)
            except WavTokError:                                       # the plan has no such buffer
                skipped.add(st)
                continue
            if st == "bb.out":
                mine = buf.view(shape).cpu()                              # (B, L, C) in both
                my_head = mine[0, :H].numpy()
            else:
                Bc, C, Tt = shape                                         # reference (B, C, T); ours (B, T, C)
                mine = buf.view(Bc, Tt, C).permute(0, 2, 1).cpu()
                my_head = mine[0, :, :H].numpy()
            ref_head = torch.from_numpy(g[f"{case}/tap/{st}/head"])
            if fmt & _capi.BUF_ELU:
                ref_head = F.elu(ref_head)
            e_head = rel_l2(my_head, ref_head.numpy())
            if path == "shipped":
                ref = orc["taps"][st]
                ref = F.elu(ref) if fmt & _capi.BUF_ELU else ref
                e_full = rel_l2(mine.numpy(), ref.numpy())
            else:
                assert fmt == 0, (st, fmt)                                # the debug twin keeps raw fp32 tensors
                l2 = float(np.sqrt((mine.numpy().astype(np.float64) ** 2).sum()))
                e_full = abs(l2 - float(g[f"{case}/tap/{st}/l2"])) / float(g[f"{case}/tap/{st}/l2"])
            report.append((st, fmt, e_head, e_full))
        worst = max(report, key=lambda r: max(r[2], r[3]))
        parity_log.record(f"arch_stage_taps[{name},{case},{path}]", worst_tap=worst[0], worst_rel_l2=max(worst[2], worst[3]),
                          taps=len(report), not_kept=",".join(sorted(skipped)))
        bad = [r for r in report if not (r[2] <= STAGE_TOL and r[3] <= STAGE_TOL)]
        assert not bad, "first diverging stage: %s (fmt %d, head rel-L2 %.3g, full %.3g); all: %s" % (*bad[0], report)
        # a tap is missing exactly where the plan fuses it into its consumer: the first conv into the stage-1 resblock, and that
        # resblock into the kernel with its down conv where the first encoder ratio has one (wide: 2, at T >= 1024)
        if path == "unfused":
            want_skipped = {"bb.pos_net.5", "head.out"}
        else:
            want_skipped = FUSED_AWAY if arch.enc_ratios[0] in (2, 4) and T >= 1024 else FUSED_AWAY - {"enc.1"}
        assert skipped == want_skipped, (skipped, want_skipped)
        assert len(report) == len(stages) - len(skipped)
    finally:
        m.set_debug_keep_stages(False)
    assert codes.dtype == torch.int64 and tuple(codes.shape) == g[f"{case}/codes"].shape == (1, B, L)
    assert check_codes(codes.cpu().numpy(), g[f"{case}/codes"], g[f"{case}/margin"], f"{name}/{case}/{path}") == 0
    _check_waveform(name, case, out.cpu().numpy(), f"{name}/{case}/{path}")
    m.check_status()


@pytest.mark.parametrize("case", A.CASES)
def test_codes_waveform_and_float64(vm, case):
    """The rule of test_precision_against_float64: the oracle runs in float64 and the CPU fp32 oracle (= the reference), the
    shipped GPU path and the GPU's plain fp32 chain are measured against it.  The shipped path's error (pre-VQ embedding and
    waveform, the same features on every side) stays within 4x the CPU fp32 oracle's own error from the same run - the
    project's bar for two fp32-class roundings of one real result - and its codes are the float64 codes."""
    from tests import parity_log
    name, m = vm
    arch, cases, g = A.variant(name)
    bw = _bw(name, case)
    o32, o64 = A.oracle_run(name, case), A.oracle64_run(name, case)
    e64, w64 = o64["emb"].numpy(), o64["wav"].numpy()
    assert torch.equal(o64["codes"], torch.from_numpy(g[f"{case}/codes"]))
    assert np.allclose(o64["margin"].numpy(), g[f"{case}/margin"], rtol=1e-6, atol=1e-6)      # the fixture's margins are float64's
    res = {"cpu_fp32_oracle": {"emb": rel_l2(o32["taps"][o64["emb_key"]].numpy(), e64), "wav": rel_l2(o32["wav"].numpy(), w64),
                               "codes_equal_fp64": bool(torch.equal(o32["codes"], o64["codes"]))}}
    wav = torch.from_numpy(A.clips(name, case)).cuda()
    for label, mode in (("gpu_f16x3_shipped", "f16x3"), ("gpu_fp32_chain", "f32")):
        m.set_gemm_precision(mode)
        try:
            emb = m.feature_extractor.encodec.encoder(wav.unsqueeze(1)).cpu().numpy()
            feats, codes = m.encode_infer(wav, bandwidth_id=bw)
            own = m.decode(feats, bandwidth_id=bw).cpu().numpy()
            wg = m.decode(o32["feats"].cuda(), bandwidth_id=bw).cpu().numpy()
            m.check_status()
        finally:
            m.set_gemm_precision("f16x3")
        assert codes.dtype == torch.int64 and tuple(codes.shape) == g[f"{case}/codes"].shape
        assert check_codes(codes.cpu().numpy(), g[f"{case}/codes"], g[f"{case}/margin"], f"{name}/{case}/{label}") == 0
        res[label] = {"emb": rel_l2(emb, e64), "wav": rel_l2(wg, w64), "codes_equal_fp64": bool(torch.equal(codes.cpu(), o64["codes"])),
                      "wav_vs_fixture": _check_waveform(name, case, own, f"{name}/{case}/{label}")}
    ratio_wav = res["gpu_f16x3_shipped"]["wav"] / res["cpu_fp32_oracle"]["wav"]
    ratio_emb = res["gpu_f16x3_shipped"]["emb"] / res["cpu_fp32_oracle"]["emb"]
    parity_log.record(f"arch_vs_float64[{name},{case}]", **{f"{k}.{kk}": vv for k, v in res.items() for kk, vv in v.items()},
                      shipped_over_cpu_fp32_wav=ratio_wav, shipped_over_cpu_fp32_emb=ratio_emb,
                      wav_rel_l2=res["gpu_f16x3_shipped"]["wav_vs_fixture"], code_flips=0, frames=int(g[f"{case}/codes"].size))
    print(f"[{name}/{case}] vs float64: {res} ratios wav {ratio_wav:.3g} emb {ratio_emb:.3g}")
    assert all(v["codes_equal_fp64"] for v in res.values()), res
    assert res["gpu_f16x3_shipped"]["wav"] < 2e-5 and res["gpu_f16x3_shipped"]["emb"] < 2e-5, res       # ... and far inside 1e-4
    assert ratio_wav < 4.0 and ratio_emb < 4.0, res


def test_launch_form_invariants(vm, tmp_path):
    """Bit-exact, whatever the launch form: clip 0 alone has the bits it has inside the `rows` batch (encode_infer, decode);
    encode_codes_many / decode_many on clips cut to (T, T - hop - 3, 1024, hop) samples give each clip the bits of its own
    single call (the mixed-length kernels share the shape arithmetic); decode_codes(codes) is decode(codes_to_features(codes));
    the packed image of the model loads into a model with the same `small` outputs."""
    import yaml
    from wavtokenizer_amd import WavTokenizer
    name, m = vm
    arch, cases, _g = A.variant(name)
    B, T, _seed, _ = cases["rows"]
    bw = _bw(name, "rows")
    hop = arch.hop
    wav = torch.from_numpy(A.clips(name, "rows")).cuda()
    feats, codes = m.encode_infer(wav, bandwidth_id=bw)
    out = m.decode(feats, bandwidth_id=bw)
    # --- one clip alone
    f1, c1 = m.encode_infer(wav[:1].contiguous(), bandwidth_id=bw)
    assert torch.equal(c1, codes[:, :1]) and torch.equal(f1, feats[:1])
    assert torch.equal(m.decode(f1, bandwidth_id=bw), out[:1])
    # --- through codes
    assert torch.equal(m.decode_codes(codes, bandwidth_id=bw), out)
    assert torch.equal(m.decode(m.codes_to_features(codes), bandwidth_id=bw), out)
    m.check_status()
    # --- clips of different lengths in one call
    lengths = (T, T - hop - 3, 1024, hop)
    cut = [wav[i, :n].contiguous() for i, n in enumerate(lengths)]
    single = [m.encode_infer(c[None], bandwidth_id=bw) for c in cut]
    many = m.encode_codes_many(cut, bandwidth_id=bw)
    assert len(many) == len(cut)
    for i, (c, (_fs, cs)) in enumerate(zip(many, single)):
        assert tuple(c.shape) == (1, 1, arch.frames(lengths[i])) and torch.equal(c, cs), (name, "encode_codes_many", i, lengths[i])
    # the mixed-length encode plan takes the stage-1 kernel that holds the down conv (first encoder ratio 2 or 4); a model
    # without it encodes the clips one at a time instead of failing at the plan's creation
    from wavtokenizer_amd import _capi
    mixed = any(k[0] == _capi.WT_PLAN_ENCODE and k[3] & _capi.WT_PLAN_FLAG_MIXED_LENGTH for k in m._engine.plans)
    assert mixed == (arch.enc_ratios[0] in (2, 4)), (name, arch.enc_ratios)
    wavs = m.decode_many([fs for fs, _cs in single], bandwidth_id=bw)
    for i, (w, (fs, _cs)) in enumerate(zip(wavs, single)):
        ws = m.decode(fs, bandwidth_id=bw)
        assert tuple(w.shape) == tuple(ws.shape) == (1, arch.frames(lengths[i]) * arch.hop_length)
        assert torch.equal(w, ws), (name, "decode_many", i, lengths[i])
    m.check_status()
    # --- the packed image
    bws = _bw(name, "small")
    small = torch.from_numpy(A.clips(name, "small")).cuda()
    fs, cs = m.encode_infer(small, bandwidth_id=bws)
    os_ = m.decode(fs, bandwidth_id=bws)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml.safe_dump({"model": {"init_args": arch.to_yaml_node()}}))
    path = str(tmp_path / "model.wtpk")
    m.save_packed(path)
    m2 = WavTokenizer.from_packed(str(cfg), path)
    f2, c2 = m2.encode_infer(small, bandwidth_id=bws)
    assert torch.equal(c2, cs) and torch.equal(f2, fs)
    assert torch.equal(m2.decode(f2, bandwidth_id=bws), os_)
    m.check_status()
    m2.check_status()


@pytest.mark.parametrize("vm", ["wide"], indirect=True)
def test_adaln_rows_are_live(vm):
    """wide has three AdaLayerNorm rows: the same features decoded under bandwidth_id 0, 1 and 2 each match the oracle under
    that id, and no two results are equal (every row is read, none twice)."""
    from tests import parity_log
    name, m = vm
    arch = A.variant(name)[0]
    assert arch.adanorm_num_embeddings == 3
    feats = A.oracle_run(name, "small")["feats"]
    orc = A.oracle(name)
    outs = []
    for i in range(arch.adanorm_num_embeddings):
        with torch.inference_mode():
            want = orc.decode(feats, torch.tensor([i])).numpy()
        got = m.decode(feats.cuda(), bandwidth_id=torch.tensor([i])).cpu().numpy()
        err = rel_l2(got, want)
        parity_log.record(f"arch_adaln_row[{name},{i}]", wav_rel_l2=err)
        assert err < WAV_REL_TOL, (i, err)
        outs.append(got)
    assert len(outs) == 3
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.array_equal(outs[i], outs[j]), (i, j)
            assert rel_l2(outs[i], outs[j]) > 100 * WAV_REL_TOL, (i, j)
    m.check_status()


@pytest.mark.parametrize("k,stride", [(18, 9), (20, 10), (32, 16)])
def test_stage1_down_conv_around_the_tile_change(k, stride):
    """The first encoder stage's down conv (32 -> 64 channels, k = 2 r taps, reflect padded) on S32 operands against float64, as
    tests/test_gpu_parity.py test_conv1d_s32_kernel: N = 64 takes the 256-row tile up to 19 taps (r = 9: the last that fits) and
    the 128-row tile from r = 10 to r = 16, the largest ratio a model loads with; lengths that are no multiple of the stride,
    more rows than one tile."""
    import ctypes
    import torch.nn.functional as F
    from oracle.cpu_ref import get_extra_padding_for_conv1d, pad1d_reflect
    from wavtokenizer_amd._capi import lib, check
    B, T, Cin, Cout = 3, 40 * stride + 7, 32, 64
    gen = torch.Generator().manual_seed(k)
    x = torch.randn(B, Cin, T, generator=gen)
    w = torch.randn(Cout, Cin, k, generator=gen) / (Cin * k) ** 0.5
    b = torch.randn(Cout, generator=gen)
    pt = k - stride
    extra = get_extra_padding_for_conv1d(T, k, stride, pt)
    pr = pt // 2
    want = F.conv1d(pad1d_reflect(x, (pt - pr, pr + extra)).double(), w.double(), b.double(), stride=stride)
    Tout = want.shape[-1]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    xg, wg, bg = x.permute(0, 2, 1).contiguous().cuda(), w.permute(0, 2, 1).contiguous().cuda(), b.cuda()
    y = torch.full((B, Tout, Cout), float("nan"), device="cuda")
    ws = torch.empty(4 * (B * T * Cin + Cout * k * Cin) + 1024, dtype=torch.uint8, device="cuda")
    check(lib.wt_conv1d_s32(ptr(xg), ptr(wg), ptr(bg), ptr(y), B, T, Cin, Cout, k, stride, 0, ptr(ws), None), "wt_conv1d_s32")
    torch.cuda.synchronize()
    assert rel_l2(y.permute(0, 2, 1).cpu().numpy(), want.numpy()) < 1e-6
