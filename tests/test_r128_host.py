"""The R 128 meter without a GPU: the new exports against the header, the refusals of the C ABI (made before any device call: the
pointers here are never read), wt_short_term_blocks against tests/r128_ref.py, the references themselves against the cases of EBU
Tech 3341 (15-18: true peak of fs / 4 sines) and Tech 3342 (1-4: loudness range of stepped tones), the rank formulas, and the
argument errors of the public calls (raised before any GPU work: the tensors here live on the CPU)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import loudness_ref as R
from tests import r128_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"wt_true_peak_tile": 0, "wt_true_peak_workspace_bytes": 2, "wt_true_peak": 5, "wt_short_term_blocks": 2,
               "wt_loudness_range_workspace_bytes": 2, "wt_loudness_range": 5, "wt_normalize_rows_lufs_tp_workspace_bytes": 2,
               "wt_normalize_rows_lufs_tp": 10}


@pytest.fixture(scope="module")
def model():
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    return WavTokenizer.from_arch(ARCH_HOP600)                 # on the CPU: nothing here may reach the GPU


def test_new_exports_match_the_header():
    from wavtokenizer_amd import _capi
    header = open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")).read()
    for name, n_args in NEW_EXPORTS.items():
        m = re.search(r"^(size_t|int|int32_t|int64_t)\s+%s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        args = [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
        assert len(args) == n_args, (name, args)
        assert name in _capi.EXPORTS
        fn = getattr(_capi.lib, name)
        assert len(fn.argtypes) == n_args, name
        if m.group(1) == "size_t":
            assert fn.restype is _capi.c_size_t, name
        if m.group(1) == "int64_t":
            assert fn.restype is _capi.c_int64, name
    assert [f for f, _t in _capi.WtTruePeakClip._fields_] == ["x", "n", "channels", "channel_stride", "out"]
    assert ctypes.sizeof(_capi.WtTruePeakClip) == 40
    assert [f for f, _t in _capi.WtLoudnessRangeClip._fields_] == ["x", "n", "channels", "channel_stride", "out", "momentary", "short_term"]
    assert ctypes.sizeof(_capi.WtLoudnessRangeClip) == 56
    for struct, fields in (("wt_true_peak_clip", _capi.WtTruePeakClip._fields_), ("wt_loudness_range_clip", _capi.WtLoudnessRangeClip._fields_)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert [re.search(r"(\w+)\s*$", d).group(1) for d in body.split(";") if d.strip()] == [f for f, _t in fields], struct
    T = int(_capi.lib.wt_true_peak_tile())
    assert T >= 64 and T % 64 == 0
    lib = _capi.lib
    assert int(lib.wt_true_peak_workspace_bytes(0, 10)) == 0 and int(lib.wt_loudness_range_workspace_bytes(0, 10)) == 0
    assert int(lib.wt_normalize_rows_lufs_tp_workspace_bytes(0, 10)) == 0
    assert int(lib.wt_loudness_range_workspace_bytes(3, 30000)) > int(lib.wt_loudness_workspace_bytes(3, 30000))
    assert int(lib.wt_normalize_rows_lufs_tp_workspace_bytes(3, 100)) > int(lib.wt_normalize_rows_lufs_workspace_bytes(3, 100))
    # the calls the new ones stand beside keep their signatures
    assert len(lib.wt_loudness.argtypes) == 5 and len(lib.wt_normalize_rows_lufs.argtypes) == 9 and ctypes.sizeof(_capi.WtLoudnessClip) == 48


def test_refusals_before_any_device_call():
    """Every call below has exactly one thing wrong and must return before it touches the device: the pointers are made up."""
    from wavtokenizer_amd import _capi
    lib, INVALID = _capi.lib, _capi.WT_ERR_INVALID
    fake = 0x10000

    def setter(j, field, value):
        return lambda descs: setattr(descs[j], field, value)

    def peak(mutate=lambda d: None, B=2, rate=24000, workspace=fake):
        descs = (_capi.WtTruePeakClip * 2)()
        for j, d in enumerate(descs):
            d.x, d.n, d.channels, d.channel_stride, d.out = fake, 9600, 1, 0, fake + 64 + 8 * j
        mutate(descs)
        return lib.wt_true_peak(descs, B, rate, ctypes.c_void_p(workspace), None)

    def rng(mutate=lambda d: None, B=2, rate=24000, workspace=fake):
        descs = (_capi.WtLoudnessRangeClip * 2)()
        for j, d in enumerate(descs):
            d.x, d.n, d.channels, d.channel_stride, d.out, d.momentary, d.short_term = fake, 96000, 1, 0, fake + 64 + 36 * j, None, None
        mutate(descs)
        return lib.wt_loudness_range(descs, B, rate, ctypes.c_void_p(workspace), None)

    for fn, call, extra in ((b"wt_true_peak", peak, ()),
                            (b"wt_loudness_range", rng, (("misaligned momentary", setter(0, "momentary", fake + 1)),
                                                         ("misaligned short_term", setter(1, "short_term", fake + 2))))):
        cases = [("B = 0", call(B=0)), ("B = 65536", call(B=65536)), ("rate 7999", call(rate=7999)), ("rate 192001", call(rate=192001)),
                 ("n = 0", call(setter(1, "n", 0))), ("n < 0", call(setter(0, "n", -3))), ("channels 0", call(setter(1, "channels", 0))),
                 ("channels 3", call(setter(0, "channels", 3))), ("null x", call(setter(1, "x", None))),
                 ("misaligned x", call(setter(0, "x", fake + 2))), ("null out", call(setter(1, "out", None))),
                 ("misaligned out", call(setter(1, "out", fake + 65))), ("null workspace", call(workspace=None)),
                 ("misaligned workspace", call(workspace=fake + 4))]
        cases += [(what, call(mutate)) for what, mutate in extra]
        for what, rc in cases:
            assert rc == INVALID, (fn, what)
            assert fn in lib.wt_last_error(), (fn, what)
    assert lib.wt_true_peak(None, 2, 24000, ctypes.c_void_p(fake), None) == INVALID
    assert lib.wt_loudness_range(None, 2, 24000, ctypes.c_void_p(fake), None) == INVALID

    def norm(n=(9600, 9600), rows=fake, T_pad=9600, rate=24000, target=-23.0, ceiling=-1.0, scales=fake + 64, workspace=fake + 128, B=2):
        return lib.wt_normalize_rows_lufs_tp(ctypes.c_void_p(rows), B, T_pad, (ctypes.c_int64 * 2)(*n), rate, target, ceiling,
                                             ctypes.c_void_p(scales), ctypes.c_void_p(workspace), None)

    for what, rc in (("n > T_pad", norm(n=(9600, 9601))), ("n = 0", norm(n=(0, 9600))), ("null rows", norm(rows=None)),
                     ("misaligned rows", norm(rows=fake + 2)), ("T_pad = 0", norm(T_pad=0)), ("rate", norm(rate=4000)),
                     ("target nan", norm(target=float("nan"))), ("ceiling nan", norm(ceiling=float("nan"))),
                     ("ceiling inf", norm(ceiling=float("inf"))), ("ceiling -inf", norm(ceiling=-float("inf"))),
                     ("null scales", norm(scales=None)), ("misaligned scales", norm(scales=fake + 66)),
                     ("null workspace", norm(workspace=None)), ("misaligned workspace", norm(workspace=fake + 4)), ("B = 0", norm(B=0))):
        assert rc == INVALID, what
        assert b"wt_normalize_rows_lufs_tp" in lib.wt_last_error(), what


def test_short_term_block_count():
    from wavtokenizer_amd import _capi
    lib = _capi.lib
    for fs in (8000, 11025, 22050, 24000, 44100, 48000, 192000):
        first = 3 * fs
        for n in (first - 1, first, first + 1, (31 * fs) // 10 - 1, (31 * fs) // 10, (31 * fs) // 10 + 1, 1, fs, 10 * fs + 7):
            S = int(lib.wt_short_term_blocks(n, fs))
            assert S == Q.short_term_blocks(n, fs), (fs, n)
            assert S == max(int(lib.wt_loudness_blocks(n, fs)) - 26, 0), (fs, n)
    assert Q.short_term_blocks(33074, 11025) == 0 and Q.short_term_blocks(33075, 11025) == 1
    assert Q.short_term_blocks(34177, 11025) == 2 and Q.short_term_blocks(34176, 11025) == 1        # floor(31 * 1102.5) = 34177
    assert int(lib.wt_short_term_blocks(0, 24000)) == 0 and int(lib.wt_short_term_blocks(10 ** 6, 100)) == 0


def test_rank_formulas_are_the_nearest_rank_points():
    """lo and hi are round-half-up of 0.10 (m - 1) and 0.95 (m - 1), in range and ordered, for m = 1 ... 41."""
    for m in range(1, 42):
        lo, hi = Q.ranks(m)
        assert lo == math.floor(0.10 * (m - 1) + 0.5 + 1e-9) and hi == math.floor(0.95 * (m - 1) + 0.5 + 1e-9), m
        assert 0 <= lo <= hi <= m - 1, m
    assert Q.ranks(1) == (0, 0) and Q.ranks(11) == (1, 10) and Q.ranks(21) == (2, 19) and Q.ranks(41) == (4, 38)


def test_reference_true_peak_reads_tech_3341_cases_15_to_18():
    """A sine at fs / 4 of amplitude 0.5 with phase 0 / 45 / 60 / 67.5 degrees: -6.0 +0.2 / -0.4 dBTP at every rate."""
    want_sample = {0.0: -6.02, 45.0: -9.03, 60.0: -7.27, 67.5: -6.71}
    want_true = {0.0: -6.021, 45.0: -5.917, 60.0: -5.997, 67.5: -5.907}
    for fs in (8000, 16000, 24000, 44100, 48000):
        assert Q.factor(fs) == 4
        for phase in want_sample:
            x = 0.5 * np.sin(2 * np.pi * 0.25 * np.arange(fs // 2) + math.radians(phase))
            tp, sp, _bound = Q.true_peak(x, fs)
            assert abs(Q.db(sp) - want_sample[phase]) <= 0.01, (fs, phase, Q.db(sp))
            assert abs(Q.db(tp) - want_true[phase]) <= 0.002, (fs, phase, Q.db(tp))
            assert -6.4 <= Q.db(tp) <= -5.8 and tp >= sp, (fs, phase)
    assert (Q.factor(95999), Q.factor(96000), Q.factor(191999), Q.factor(192000)) == (4, 2, 2, 1)
    for F in (4, 2):
        h = Q.taps(F)
        assert h.dtype == np.float32 and h.shape == (49,) and h[0] == 0 and abs(h[48]) < 1e-7 and h[24] == 1
        assert max(np.abs(h[p:48:F]).sum() for p in range(1, F)) < (1.87 if F == 4 else 2.31)  # (test_r128_calls.py's slack uses the first)
    x = np.array([0.25, -0.75, 0.5])
    assert Q.true_peak(x, 192000) == (0.75, 0.75, 0.0)


def test_reference_loudness_range_reads_tech_3342_cases_1_to_4():
    for levels, want in (((-20, -30), 10.0), ((-20, -15), 5.0), ((-40, -20), 20.0), ((-50, -35, -20, -35, -50), 15.0)):
        z, s = Q.short_term(Q.tone_levels(levels), 48000)
        assert len(z) == 10 * 20 * len(levels) - 29
        lra, lo, hi, m, _rel, _margin = Q.loudness_range(z)
        assert abs(lra - want) <= 0.01, (levels, lra)                      # (the cases ask for +- 1 LU)
        assert m > 0 and lo < hi
    # nothing to range over: under 3 s, silence, all under -70
    assert Q.short_term(np.zeros(71999), 24000)[0].shape == (0,)
    for x in (np.zeros(80000), 1e-6 * np.random.default_rng(0).standard_normal(80000)):
        lra, lo, hi, m, _rel, _margin = Q.loudness_range(Q.short_term(x, 24000)[0])
        assert math.isnan(lra) and math.isnan(lo) and math.isnan(hi) and m == 0


def test_ceiling_arguments_raise_before_any_gpu_work(model):
    from wavtokenizer_amd import audio
    wav = torch.zeros(1, 12000)
    clips = [torch.zeros(12000)]
    calls = {
        "normalize": lambda **kw: audio.normalize(wav, kw.pop("normalize", "peak"), **kw),
        "encode_codes": lambda **kw: model.encode_codes(wav, **kw),
        "encode_codes_many": lambda **kw: model.encode_codes_many(clips, **kw),
        "encode_codes_segmented": lambda **kw: model.encode_codes_segmented(clips[0], 1200, 600, **kw),
        "encode_codes_segmented_many": lambda **kw: model.encode_codes_segmented_many(clips, 1200, 600, **kw),
    }
    for name, call in calls.items():
        for kw in (dict(max_true_peak_db=-1.0), dict(normalize="peak", max_true_peak_db=-1.0), dict(normalize="rms", max_true_peak_db=-1),
                   dict(normalize="lufs", max_true_peak_db=float("nan")), dict(normalize="lufs", max_true_peak_db=float("inf")),
                   dict(normalize="lufs", max_true_peak_db=True), dict(normalize="lufs", max_true_peak_db="-1")):
            if name == "normalize" and "normalize" not in kw:
                continue                                                   # (audio.normalize always has a mode)
            with pytest.raises(ValueError, match="max_true_peak_db"):
                call(**kw)
    with pytest.raises(TypeError):                                         # keyword-only
        audio.normalize(wav, "lufs", 0.0, -1.0)
    with pytest.raises(ValueError, match="max_true_peak_db"):
        audio.normalize_rows(torch.zeros(1, 100), [100], 0, 1.0, max_true_peak_db=-1.0)
    # None leaves normalize_args and its two-value result as they were
    assert audio.ceiling_arg("x", None, None) is None and audio.ceiling_arg("x", "peak", None) is None
    assert audio.ceiling_arg("x", "lufs", -1) == -1.0 and isinstance(audio.ceiling_arg("x", "lufs", -1), float)
    assert audio.normalize_args("x", "lufs", 0.0, -16.0) == (2, -16.0) and audio.normalize_args("x", None, 0.0) is None
    assert len(audio.normalize_args("x", "peak", -3.0)) == 2


def test_measuring_calls_refuse_cpu_tensors_and_bad_arguments():
    from wavtokenizer_amd import audio, metrics
    x = torch.zeros(96000)
    for call in (lambda: audio.true_peak(x, 24000), lambda: audio.true_peak_many([x], 24000), lambda: audio.loudness_range(x, 24000),
                 lambda: audio.loudness_range_many([x], 24000, series=True), lambda: audio.r128_many([x], 24000),
                 lambda: metrics.loudness_range_delta(x, x, 24000), lambda: metrics.true_peak_delta(x, x, 24000),
                 lambda: audio.normalize(x, "lufs", max_true_peak_db=-1.0)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    for fn in (audio.true_peak_many, audio.loudness_range_many, audio.r128_many):
        for args in (([],), ([x], 4000), ([x], [24000, 24000]), ([x], True), ([x.double()],), ([torch.zeros(3, 100)],), ([torch.zeros(0)],)):
            with pytest.raises(ValueError):
                fn(*args)
    for fn in (metrics.loudness_range_delta_many, metrics.true_peak_delta_many):
        with pytest.raises(ValueError):
            fn([x], [x, x])
        with pytest.raises(ValueError):
            fn([], [])
        with pytest.raises(ValueError):
            fn([x], [x], sample_rate=[24000, 24000])
