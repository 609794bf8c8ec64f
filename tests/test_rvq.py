"""Residual VQ encode on the GPU, on three-codebook models: the derived tables of codebooks 1 and 2 (wt_model_codebook_tables), the
WT_PLAN_QUANTIZE plan against the fixture captured from the reference (tests/golden/hop600_rvq3.npz) and the teacher-forced check of
tests/rvq_ref.py, WT_PLAN_FLAG_RVQ encode plans through encode_codes(n_q=...) / encode_codes_many(n_q=...) plain, graph-replayed and
mixed-length, and the refusals.  Two models: hop600 with the fixture's weights, and a small twin with vq_bins = 100 whose codebooks
1 and 2 hold exact duplicate rows."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import f16_ref, ingest_ref
from tests import rvq_ref as R
from tests import vq_ref as V
from tests import weights_ref as W
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

VQ = "feature_extractor.encodec.quantizer.vq.layers.%d._codebook.embed"
DUPS = {1: (5, 40), 2: (7, 90)}          # twin: codebook k's row c is repeated at c' > c
_MODELS = {}


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(GOLDEN + "/hop600_rvq3.npz")


def _arch(name):
    from wavtokenizer_amd import ARCH_HOP600
    return dataclasses.replace(ARCH_HOP600, num_quantizers=3, **({"vq_bins": 100} if name == "twin" else {}))


@functools.lru_cache(maxsize=None)
def _sd(name):
    from wavtokenizer_amd import synth
    sd = synth.make_state_dict(_arch(name), seed=int(gold()["weight_seed"]))
    if name == "twin":
        for k, (c, c2) in DUPS.items():
            sd[VQ % k] = sd[VQ % k].copy()
            sd[VQ % k][c2] = sd[VQ % k][c]
    return sd


def _model(name):
    from wavtokenizer_amd import WavTokenizer
    if name not in _MODELS:
        m = WavTokenizer.from_arch(_arch(name))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(name).items()}, strict=False)
        m = m.eval().to("cuda")
        m._ensure_engine()
        _MODELS[name] = m
    return _MODELS[name]


@functools.lru_cache(maxsize=None)
def _books(name):
    books = [torch.from_numpy(_sd(name)[VQ % k]) for k in range(3)]
    return books, [V.host_serial_ee(e) for e in books]


def _quiet(m):
    m.check_status()
    assert not m.fallback_events


def _lib():
    from wavtokenizer_amd import _capi
    return _capi.lib


@functools.lru_cache(maxsize=None)
def _hip():
    lib = ctypes.CDLL("libamdhip64.so")
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return lib


def _read(ptr, words):
    torch.cuda.synchronize()
    host = np.empty(words, np.uint32)
    assert _hip().hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), words * 4, 2) == 0      # device to host
    return host


def _listing(model):
    from wavtokenizer_amd._capi import WtWeightInfo
    out = []
    for i in range(_lib().wt_model_weight_count(model)):
        w = WtWeightInfo(size=ctypes.sizeof(WtWeightInfo))
        assert _lib().wt_model_weight_info(model, i, ctypes.byref(w)) == 0
        out.append((w.name.decode(), w.data, w.numel, w.format, w.acc_scale, w.alloc))
    return out


def _tables(model, k):
    s32, ee, acc = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
    rc = _lib().wt_model_codebook_tables(model, k, ctypes.byref(s32), ctypes.byref(ee), ctypes.byref(acc))
    assert rc == 0, _lib().wt_last_error().decode()
    return s32.value, ee.value, acc.value


def _wav(B, T, seed):
    from wavtokenizer_amd import synth
    return torch.from_numpy(synth.make_clips(B, T, seed=seed)).cuda()


def _plans(m, pred):
    return [(k, p) for k, (p, _ws) in m._engine.plans.items() if pred(k)]


# ------------------------------------------------------------------------------------------------ derived tables
def test_codebook_tables_are_derived_state():
    """A model of its own (no residual VQ plan has touched it): the listing and the packed image are the same before and after the
    tables are built; k = 0 is the listed arrays; k = 1, 2 are the split of E_k by vq.embed.s32's rule and the host's serial sums."""
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.pretrained import _Engine
    arch, sd = _arch("twin"), _sd("twin")
    e = _Engine()
    e.load(arch, {k: torch.from_numpy(v) for k, v in sd.items()}, torch.cuda.current_device())
    before, image = _listing(e.model), e.export().copy()
    by_name = {n: (p, numel, acc) for n, p, numel, _f, acc, _a in before}
    s32, ee, acc = _tables(e.model, 0)
    assert (s32, acc) == (by_name["vq.embed.s32"][0], by_name["vq.embed.s32"][2]) and ee == by_name["vq.ee"][0]
    bins, seen = arch.vq_bins, {p for _n, p, *_r in before}
    for k in (1, 2):
        s32, ee, acc = _tables(e.model, k)
        assert s32 and ee and s32 not in seen and ee not in seen
        assert _tables(e.model, k) == (s32, ee, acc), "built once"
        Ek = sd[VQ % k]
        s = f16_ref.s32_weight_scale(float(np.abs(Ek).max()))
        assert s != 0.0 and acc == 1.0 / s
        words = _read(s32, bins * 512).view(np.uint16)
        assert W.same_words(words, W.split_emulate((Ek * np.float32(s)).reshape(-1)), s32=True), f"codebook {k}: S32 words"
        got_ee = _read(ee, bins)
        assert np.array_equal(got_ee, V.host_serial_ee(torch.from_numpy(Ek)).numpy().view(np.uint32)), f"codebook {k}: |e|^2"
    for bad in (-1, 3):
        assert _lib().wt_model_codebook_tables(e.model, bad, None, None, None) == _capi.WT_ERR_INVALID
    assert _listing(e.model) == before and np.array_equal(e.export(), image)
    e.close()


def test_codebook_tables_of_the_fixture_model():
    m = _model("fix")
    books, ees = _books("fix")
    before = _listing(m._engine.model)
    for k in (1, 2):
        s32, ee, acc = _tables(m._engine.model, k)
        Ek = books[k].numpy()
        s = f16_ref.s32_weight_scale(float(np.abs(Ek).max()))
        assert acc == 1.0 / s
        assert W.same_words(_read(s32, Ek.size).view(np.uint16), W.split_emulate((Ek * np.float32(s)).reshape(-1)), s32=True)
        assert np.array_equal(_read(ee, Ek.shape[0]), ees[k].numpy().view(np.uint32))
    assert _listing(m._engine.model) == before


# ------------------------------------------------------------------------------------------- WT_PLAN_QUANTIZE
@pytest.mark.parametrize("route", ["f16x3", "f32"])
def test_quantize_on_the_fixture(route):
    """The reference's emb through quantizer.encode: the fixture's codes outside undecidable frames (at most 5 % of them), the
    teacher-forced check in every round, K from the bandwidth, and the prefix property."""
    m = _model("fix")
    g = gold()
    books, ees = _books("fix")
    emb = torch.from_numpy(g["emb"]).cuda()
    rows = R.rows_of(torch.from_numpy(g["emb"]))
    kernel = 0 if route == "f16x3" else 1
    q = m.feature_extractor.encodec.quantizer
    try:
        m.set_gemm_precision(route)
        full = q.encode(emb, int(g["frame_rate"]), None)
        assert full.shape == (3, 2, 40) and full.dtype == torch.int64
        left = R.check_against(full.cpu(), torch.from_numpy(g["all/codes"]), rows, books, kernel, ees, what=route)
        res = R.check_teacher_forced(full.cpu(), rows, books, kernel, ees, what=route)
        print(f"{route}: {left} of 80 frames left out; decidable rows per round {[s for s, _n in res]}")
        for tag, bw, K in (("bw0p6", 0.6, 2), ("bw0p1", 0.1, 1)):
            c = q.encode(emb, int(g["frame_rate"]), bw)
            assert c.shape == (K, 2, 40) and torch.equal(c, full[:K]), tag
            R.check_against(c.cpu(), torch.from_numpy(g[f"{tag}/codes"]), rows, books, kernel, ees, what=f"{route} {tag}")
        assert q.encode(emb, int(g["frame_rate"]), 100.0).shape[0] == 3                 # above all layers: cut to them
    finally:
        m.set_gemm_precision("f16x3")
    _quiet(m)


def _designed(books, ees, kernel, n):
    """Rows x = fl(E_0[a] + E_1[c]) with c duplicated at c' > c: round 0 gives a (asserted here: decidable, and a), round 1 must
    give c, the lower of two bit-identical rows."""
    c, c2 = DUPS[1]
    assert torch.equal(books[1][c], books[1][c2])
    x = torch.stack([books[0][a] + books[1][c] for a in range(11, 11 + n)])
    ref = V.Ref(x, books[0], kernel, ees[0])
    und, ok = V.undecidable(ref)
    assert und == 0 and ok == n, "precondition: round 0 of the designed rows is decidable"
    assert ref.d.argmax(-1).tolist() == list(range(11, 11 + n)), "precondition: round 0 gives a"
    return x, list(range(11, 11 + n)), c


@pytest.mark.parametrize("B,L", [(1, 1), (3, 33), (2, 64), (1, 257)])
@pytest.mark.parametrize("route", ["f16x3", "f32"])
def test_quantize_shapes_on_the_twin(route, B, L):
    m = _model("twin")
    books, ees = _books("twin")
    kernel = 0 if route == "f16x3" else 1
    gen = torch.Generator().manual_seed(100 * B + L)
    # seeded rows near sums of one row per codebook, so that every round has something to find
    pick = torch.randint(0, 100, (3, B * L), generator=gen)
    x = books[0][pick[0]] + books[1][pick[1]] + 0.5 * books[2][pick[2]] + 0.05 * torch.randn(B * L, 512, generator=gen)
    n_des = min(4, B * L - 1) if B * L > 1 else 1
    des, want_a, want_c = _designed(books, ees, kernel, n_des)
    x[:n_des] = des
    feats = x.reshape(B, L, 512).transpose(1, 2).contiguous().cuda()
    q = m.feature_extractor.encodec.quantizer
    try:
        m.set_gemm_precision(route)
        codes = q.encode(feats, 25)
        again = q.encode(feats, 25)              # B <= 16: the second call records, this one and the next replay
        third = q.encode(feats, 25, 0.4)         # 100 bins at frame rate 25: 166.1 per codebook, K = floor(400 / 166.1) = 2
    finally:
        m.set_gemm_precision("f16x3")
    assert codes.shape == (3, B, L) and third.shape == (2, B, L) and torch.equal(codes, again) and torch.equal(third, codes[:2])
    flat = codes.cpu().reshape(3, -1)
    res = R.check_teacher_forced(flat, x, books, kernel, ees, what=f"{route} {B}x{L}")
    assert all(n == B * L for _s, n in res) and sum(n - s for s, n in res) <= R.MAX_UNDECIDABLE * 3 * B * L
    assert flat[0, :n_des].tolist() == want_a and flat[1, :n_des].tolist() == [want_c] * n_des, "designed rows"
    _quiet(m)


# --------------------------------------------------------------------------------- WT_PLAN_FLAG_RVQ encode plans
@functools.lru_cache(maxsize=None)
def _fixture_wav():
    return _wav(2, 24000, int(gold()["clip_seed"]))


def test_prefix_and_row_zero_through_encode_codes():
    m = _model("fix")
    wav = _fixture_wav()
    c3 = m.encode_codes(wav, n_q=3)
    c2 = m.encode_codes(wav, n_q=2)
    c1 = m.encode_codes(wav, n_q=1)
    c0 = m.encode_codes(wav)
    assert c3.shape == (3, 2, 40) and c2.shape == (2, 2, 40) and c0.shape == (1, 2, 40) and c3.dtype == torch.int64
    assert torch.equal(c3[:2], c2) and torch.equal(c3[:1], c1) and torch.equal(c3[:1], c0)
    assert torch.equal(c0, m.encode_infer(wav, bandwidth_id=torch.tensor([0]))[1])
    assert all(int(c3[k].unique().numel()) > 20 for k in range(3))
    # the encoder output of this plan against the residual rounds: teacher-forced on the plan's own emb
    emb = m.feature_extractor.encodec.encoder(wav[:, None, :])
    books, ees = _books("fix")
    R.check_teacher_forced(c3.cpu().reshape(3, -1), R.rows_of(emb.cpu()), books, 0, ees, what="encode_codes(n_q=3)")
    _quiet(m)


def test_batch_invariance():
    """A clip alone and in slot 2 of a batch of five gives the same words."""
    m = _model("fix")
    five = _wav(5, 9000, seed=41)
    alone = m.encode_codes(five[2:3], n_q=3)
    batch = m.encode_codes(five, n_q=3)
    assert torch.equal(batch[:, 2:3], alone)
    _quiet(m)


def _run_raw(m, kind, B, length, flags, n_q, x, fill):
    """One plan of its own through the C entry points on a workspace pre-filled with `fill` (a 32-bit pattern) before every
    call: the codes of a direct call and, for a graph plan, of the recording call and a replay."""
    from wavtokenizer_amd import _capi
    lib = _lib()
    plan = ctypes.c_void_p()
    assert lib.wt_plan_create_ex(m._engine.model, kind, B, length, flags, 0, ctypes.byref(plan)) == 0, lib.wt_last_error().decode()
    L = lib.wt_plan_frames(plan)
    n = lib.wt_plan_workspace_bytes(plan)
    ws = torch.empty(n // 4, dtype=torch.int32, device="cuda")
    codes = torch.empty((n_q, B, L), dtype=torch.int64, device="cuda")
    entry = lib.wt_quantize if kind == _capi.WT_PLAN_QUANTIZE else lib.wt_encode_rvq
    out = []
    for _call in range(3 if flags & _capi.WT_PLAN_FLAG_GRAPH else 1):
        ws.fill_(fill)
        codes.fill_(-7)
        rc = entry(plan, x.data_ptr(), n_q, codes.data_ptr(), ws.data_ptr(), None)
        assert rc == 0, lib.wt_last_error().decode()
        torch.cuda.synchronize()
        out.append(codes.cpu().clone())
    replays = lib.wt_plan_graph_replays(plan)
    bits = ctypes.c_int32()
    assert lib.wt_plan_status(plan, ctypes.byref(bits), 1) == 0 and bits.value == 0
    lib.wt_plan_destroy(plan)
    if flags & _capi.WT_PLAN_FLAG_GRAPH:
        assert replays == 2
    return out


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("what", ["quantize", "encode"])
def test_nothing_of_the_workspace_is_read_before_it_is_written(what, graph):
    """A workspace of NaN bits and one of 0xAA bytes give the codes of a zero-filled one, direct and under graph replay, for a call
    that runs all three rounds and for one that stops after two (the third round's buffers then stay unwritten)."""
    from wavtokenizer_amd import _capi
    m = _model("fix")
    with torch.cuda.stream(torch.cuda.default_stream()):
        if what == "quantize":
            kind, B, length, x = _capi.WT_PLAN_QUANTIZE, 2, 40, torch.from_numpy(gold()["emb"]).cuda()
        else:
            kind, B, length, x = _capi.WT_PLAN_ENCODE, 2, 9000, _wav(2, 9000, seed=17)
        flags = (_capi.WT_PLAN_FLAG_RVQ if what == "encode" else 0) | (_capi.WT_PLAN_FLAG_GRAPH if graph else 0)
        for n_q in (3, 2):
            base = _run_raw(m, kind, B, length, flags, n_q, x, 0)
            assert all(torch.equal(b, base[0]) for b in base) and int(base[0].min()) >= 0
            for fill in (0x7FC00000, -1431655766):           # NaN bits, 0xAAAAAAAA
                got = _run_raw(m, kind, B, length, flags, n_q, x, fill)
                assert all(torch.equal(c, base[0]) for c in got), (what, graph, n_q, hex(fill & 0xFFFFFFFF))
    _quiet(m)


def test_n_q_is_an_argument_of_the_call_and_of_the_graph_key():
    """B = 2: calls with n_q = 3, 2, 3 in a row on ONE graph plan give the bits of plans that never record."""
    from wavtokenizer_amd import _capi
    m = _model("fix")
    wav = _wav(2, 7000, seed=23)
    rvq = lambda k: k[0] == _capi.WT_PLAN_ENCODE and k[3] & _capi.WT_PLAN_FLAG_RVQ and k[1] == 2 and k[2] == 7000
    try:
        m.set_graph_max_clips(0)
        want = {n: m.encode_codes(wav, n_q=n) for n in (2, 3)}
        assert all(not k[3] & _capi.WT_PLAN_FLAG_GRAPH for k, _p in _plans(m, rvq))
    finally:
        m.set_graph_max_clips(16)
    assert torch.equal(want[3][:2], want[2])
    for n in (3, 2, 3, 3, 3, 2, 2, 2, 3, 2, 3):
        assert torch.equal(m.encode_codes(wav, n_q=n), want[n]), n
    (key, plan), = [(k, p) for k, p in _plans(m, rvq) if k[3] & _capi.WT_PLAN_FLAG_GRAPH]
    assert _lib().wt_plan_graph_replays(plan) >= 3
    _quiet(m)


def test_mixed_length_rows():
    """Clips of 1024, 7411 and 24000 samples in one wt_encode_rvq_mixed: each has the words of its own encode_codes(n_q=3) in all
    three rows and -1 past its frames; a clip of length 0 gets three rows of -1 without disturbing the others."""
    m = _model("fix")
    dev = m._ensure_engine()
    lengths = [1024, 7411, 24000]
    wavs = [_wav(1, n, seed=60 + i)[0] for i, n in enumerate(lengths)]
    own = [m.encode_codes(w[None], n_q=3) for w in wavs]

    def call(lens, clips, n_q=3):
        def fill(buf):
            buf.fill_(float("nan"))                         # samples past a clip's length are never read
            for j, (w, n) in enumerate(zip(clips, lens)):
                buf[j, :n].copy_(w[:n])
        (codes,), _plan = m._encode_rvq_mixed(len(lens), 24000, fill, lens, n_q, dev)
        return codes

    codes = call(lengths, wavs)
    assert codes.shape == (3, 3, 40)
    for j, n in enumerate(lengths):
        Lj = m.arch.frames(n)
        assert torch.equal(codes[:, j:j + 1, :Lj], own[j]), n
        assert bool((codes[:, j, Lj:] == -1).all()), n
    assert torch.equal(call(lengths, wavs, n_q=2), codes[:2])
    assert torch.equal(call(lengths, wavs), codes)           # (the third call in a row with these buffers: a replay)
    with_zero = call([1024, 0, 7411, 24000], [wavs[0], wavs[0], wavs[1], wavs[2]])
    assert bool((with_zero[:, 1] == -1).all())
    for j, src in ((0, 0), (2, 1), (3, 2)):
        assert torch.equal(with_zero[:, j], codes[:, src])
    _quiet(m)


def test_encode_codes_many_is_the_loop_of_encode_codes():
    """Five clips at two rates, one of them stereo int16, list and packed forms, against encode_codes(n_q=3) on convert_audio's
    output; one of them under the mixed-length minimum (it runs alone)."""
    from wavtokenizer_amd import audio
    m = _model("fix")
    rows = [(ingest_ref.make_clip(24000, 1, "mono", "f32", 9000, seed=1), 24000, "mono"),
            (ingest_ref.make_clip(16000, 1, "mono", "f32", 11000, seed=2).cuda(), 16000, "mono"),
            (ingest_ref.make_clip(16000, 2, "planar", "i16", 5000, seed=3), 16000, "planar"),
            (ingest_ref.make_clip(24000, 1, "mono", "f32", 700, seed=4), 24000, "mono"),
            (ingest_ref.make_clip(24000, 1, "mono", "f32", 20000, seed=5).cuda(), 24000, "mono")]
    want = []
    for clip, rate, layout in rows:
        x = clip.cuda()
        x = x.float() / 32768 if x.dtype == torch.int16 else x
        planar = x[None] if layout == "mono" else x
        wav = audio.convert_audio(planar.contiguous()[None], rate, ingest_ref.CODEC_RATE)[0]
        want.append(m.encode_codes(wav, n_q=3))
    clips, rates = [r[0] for r in rows], [r[1] for r in rows]
    out = m.encode_codes_many(clips, sample_rates=rates, n_q=3)
    assert len(out) == 5
    for i, (o, w) in enumerate(zip(out, want)):
        assert o.dtype == torch.int64 and o.shape == w.shape == (3, 1, w.shape[-1]) and torch.equal(o, w), i
    flat, offs = m.encode_codes_many(clips, sample_rates=rates, packed=True, n_q=3)
    assert offs.tolist() == np.concatenate([[0], np.cumsum([w.shape[-1] for w in want])]).tolist()
    assert flat.shape == (3, offs[-1]) and torch.equal(flat, torch.cat([w[:, 0, :] for w in want], dim=1))
    assert all(o.data_ptr() == out[0].data_ptr() + 8 * int(offs[i]) for i, o in enumerate(out)), "views into one [n_q][sum L] tensor"
    one = m.encode_codes_many(clips, sample_rates=rates)                                # n_q=None keeps its own layout
    assert all(torch.equal(o, w[:1]) for o, w in zip(one, want))
    _quiet(m)


def test_round_trip_meets_the_decode_side():
    m = _model("fix")
    wav = _fixture_wav()
    codes = m.encode_codes(wav, n_q=3)
    bw = torch.tensor([0])
    a = m.decode_codes(codes, bandwidth_id=bw)
    b = m.decode(m.codes_to_features(codes), bandwidth_id=bw)
    assert a.shape == (2, 24000) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    _quiet(m)


def test_off_the_shipped_route():
    """fp32 GEMMs: the rounds run on gemm.hip (teacher-forced with its bound on the plan's own emb) and encode_codes_many sends every
    clip alone; debug taps (KEEP_STAGES, no buffer aliased) and the range report launch the default kernels: the same words."""
    m = _model("fix")
    books, ees = _books("fix")
    wav = _wav(2, 9000, seed=77)
    want = m.encode_codes(wav, n_q=3)
    try:
        m.set_gemm_precision("f32")
        got = m.encode_codes(wav, n_q=3)
        emb = m.feature_extractor.encodec.encoder(wav[:, None, :])
        R.check_teacher_forced(got.cpu().reshape(3, -1), R.rows_of(emb.cpu()), books, 1, ees, what="fp32 encode_codes(n_q=3)")
        assert torch.equal(got[:2], m.encode_codes(wav, n_q=2)) and torch.equal(got[:1], m.encode_codes(wav))
        many = m.encode_codes_many([wav[0], wav[1, :5000]], n_q=3)
        assert torch.equal(many[0], got[:, :1]) and torch.equal(many[1], m.encode_codes(wav[1:2, :5000], n_q=3))
        m.set_gemm_precision("f16x3")
        m.set_debug_keep_stages(True)
        assert torch.equal(m.encode_codes(wav, n_q=3), want) and torch.equal(m.encode_codes(wav, n_q=2), want[:2])
    finally:
        m.set_gemm_precision("f16x3")
        m.set_debug_keep_stages(False)
    from wavtokenizer_amd import _capi
    for flag in (_capi.WT_PLAN_FLAG_RANGE_REPORT, _capi.WT_PLAN_FLAG_KEEP_STAGES | _capi.WT_PLAN_FLAG_RANGE_REPORT):
        for n_q in (3, 2):
            got, = _run_raw(m, _capi.WT_PLAN_ENCODE, 2, 9000, _capi.WT_PLAN_FLAG_RVQ | flag, n_q, wav, -1431655766)
            assert torch.equal(got, want[:n_q].cpu()), (flag, n_q)
    _quiet(m)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from wavtokenizer_amd import _capi
    m = _model("twin")
    lib, model = _lib(), m._engine.model
    INV = _capi.WT_ERR_INVALID

    def plan_of(kind, length, flags):
        p = ctypes.c_void_p()
        rc = lib.wt_plan_create_ex(model, kind, 1, length, flags, 0, ctypes.byref(p))
        return rc, p

    rc, rvq = plan_of(_capi.WT_PLAN_ENCODE, 2400, _capi.WT_PLAN_FLAG_RVQ)
    assert rc == 0
    rc, plain = plan_of(_capi.WT_PLAN_ENCODE, 2400, 0)
    assert rc == 0
    rc, quant = plan_of(_capi.WT_PLAN_QUANTIZE, 4, 0)
    assert rc == 0
    wav = _wav(1, 2400, seed=1)
    feats = torch.zeros(1, 512, 4, device="cuda")
    codes = torch.full((3, 1, 4), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(lib.wt_plan_workspace_bytes(p) for p in (rvq, plain, quant)), dtype=torch.uint8, device="cuda")
    a = lambda t: t.data_ptr()
    assert lib.wt_encode(rvq, a(wav), None, a(codes), None, a(ws), None) == INV and "wt_encode_rvq" in lib.wt_last_error().decode()
    assert lib.wt_encode_rvq(plain, a(wav), 1, a(codes), a(ws), None) == INV
    assert lib.wt_encode_rvq(quant, a(wav), 1, a(codes), a(ws), None) == INV
    assert lib.wt_encode_rvq_mixed(rvq, a(wav), a(wav), 1, a(codes), a(ws), None) == INV
    assert lib.wt_quantize(rvq, a(feats), 1, a(codes), a(ws), None) == INV
    assert lib.wt_encode_mixed(rvq, a(wav), a(wav), None, a(codes), None, a(ws), None) == INV
    for bad in (0, 4, -1):
        assert lib.wt_encode_rvq(rvq, a(wav), bad, a(codes), a(ws), None) == INV and "n_q" in lib.wt_last_error().decode()
        assert lib.wt_quantize(quant, a(feats), bad, a(codes), a(ws), None) == INV
    torch.cuda.synchronize()
    assert bool((codes == -7).all()), "a refused call launches nothing"
    for p in (rvq, plain, quant):
        lib.wt_plan_destroy(p)
    # flags that mean nothing to the quantize plan are refused by name; the RVQ flag belongs to encode plans
    for flag, name in ((_capi.WT_PLAN_FLAG_UNFUSED, "UNFUSED"), (_capi.WT_PLAN_FLAG_STEP_LSTM, "STEP_LSTM"), (_capi.WT_PLAN_FLAG_F16_GEMM, "F16_GEMM"),
                       (_capi.WT_PLAN_FLAG_MIXED_LENGTH, "MIXED_LENGTH"), (_capi.WT_PLAN_FLAG_RVQ, "RVQ")):
        rc, p = plan_of(_capi.WT_PLAN_QUANTIZE, 4, flag)
        assert rc == INV and name in lib.wt_last_error().decode(), name
    assert plan_of(_capi.WT_PLAN_DECODE, 4, _capi.WT_PLAN_FLAG_RVQ)[0] == INV
    for flag in (_capi.WT_PLAN_FLAG_KEEP_STAGES, _capi.WT_PLAN_FLAG_RANGE_REPORT, _capi.WT_PLAN_FLAG_FP32_GEMM, _capi.WT_PLAN_FLAG_GRAPH):
        rc, p = plan_of(_capi.WT_PLAN_QUANTIZE, 4, flag)
        assert rc == 0, lib.wt_last_error().decode()
        lib.wt_plan_destroy(p)
    with pytest.raises(_capi.WavTokError, match="n_q must be between"):
        m.encode_codes(wav, n_q=4)
    with pytest.raises(ValueError, match="codebook width"):
        m.feature_extractor.encodec.quantizer.encode(torch.zeros(1, 256, 4, device="cuda"), 25)
    _quiet(m)
