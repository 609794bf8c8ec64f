"""Loudness in LUFS without a GPU: the new exports against the header, the host-only entry points (K-weighting coefficients, block
count) against tests/loudness_ref.py, the refusals of the C ABI (made before any device call: the pointers here are never read),
the argument errors of the public calls (raised before any GPU work: the model here lives on the CPU, where any GPU work would
raise RuntimeError instead), and the reference itself against the check of the standard: a full-scale 997 Hz sine reads -3.01 LUFS."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import loudness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"wt_loudness_chunk": 0, "wt_loudness_blocks": 2, "wt_kweight_coefficients": 2, "wt_loudness_workspace_bytes": 2,
               "wt_loudness": 5, "wt_normalize_rows_lufs_workspace_bytes": 2, "wt_normalize_rows_lufs": 9}
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0 b1 b2 a1 a2 of the first stage, a1 a2 of the second
TABLE = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621)


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
    assert re.search(r"int\s+wt_loudness\(const wt_loudness_clip\* clips, int32_t B, int32_t sample_rate, void\* workspace, void\* stream\);",
                     header)
    fields = [f for f, _t in _capi.WtLoudnessClip._fields_]
    assert fields == ["x", "n", "channels", "channel_stride", "out", "blocks"] and ctypes.sizeof(_capi.WtLoudnessClip) == 48
    C = int(_capi.lib.wt_loudness_chunk())
    assert 1 <= C <= 800                                       # a chunk holds at most one 100 ms boundary at 8 kHz
    assert int(_capi.lib.wt_loudness_workspace_bytes(0, 10)) == 0 and int(_capi.lib.wt_normalize_rows_lufs_workspace_bytes(0, 10)) == 0
    assert int(_capi.lib.wt_normalize_rows_lufs_workspace_bytes(3, 100)) > int(_capi.lib.wt_loudness_workspace_bytes(3, 300))
    # wt_normalize_rows keeps its signature and its two modes
    assert len(_capi.lib.wt_normalize_rows.argtypes) == 9 and "WT_NORM_PEAK = 0, WT_NORM_RMS = 1 }" in header


def test_kweighting_coefficients():
    from wavtokenizer_amd import _capi
    out = (ctypes.c_double * 10)()
    assert _capi.lib.wt_kweight_coefficients(48000, out) == 0
    got = [out[i] for i in (0, 1, 2, 3, 4, 8, 9)]
    assert max(abs(g - t) for g, t in zip(got, TABLE)) <= 1e-12
    assert [out[5], out[6], out[7]] == [1.0, -2.0, 1.0]
    want = R.coefficients10(48000)
    assert max(abs(want[i] - t) for i, t in zip((0, 1, 2, 3, 4, 8, 9), TABLE)) <= 1e-12     # (and so does the reference)
    for fs in (8000, 11025, 16000, 22050, 24000, 44100, 96000, 192000):
        assert _capi.lib.wt_kweight_coefficients(fs, out) == 0
        want = R.coefficients10(fs)
        for i in range(10):
            assert abs(out[i] - want[i]) <= 1e-13 * abs(want[i]), (fs, i, out[i], want[i])
    for fs in (7999, 192001, 0, -1):
        assert _capi.lib.wt_kweight_coefficients(fs, out) == _capi.WT_ERR_INVALID
    assert _capi.lib.wt_kweight_coefficients(48000, None) == _capi.WT_ERR_INVALID


def test_block_count():
    from wavtokenizer_amd import _capi
    for fs in (8000, 11025, 24000, 48000):
        for n in (int(0.4 * fs) - 1, int(0.4 * fs), int(0.4 * fs) + 1, int(0.5 * fs) - 1, int(0.5 * fs), 1, 10 ** 6):
            assert int(_capi.lib.wt_loudness_blocks(n, fs)) == R.blocks(n, fs), (fs, n)
    assert R.blocks(4410, 11025) == 1 and R.blocks(4409, 11025) == 0 and R.blocks(5512, 11025) == 2 and R.blocks(5511, 11025) == 1
    assert int(_capi.lib.wt_loudness_blocks(0, 24000)) == 0 and int(_capi.lib.wt_loudness_blocks(10 ** 6, 100)) == 0


def test_refusals_before_any_device_call():
    """Every call below has exactly one thing wrong and must return before it touches the device: the pointers are made up."""
    from wavtokenizer_amd import _capi
    lib, INVALID = _capi.lib, _capi.WT_ERR_INVALID
    fake = 0x10000

    def call(mutate=lambda d: None, B=2, rate=24000, workspace=fake):
        descs = (_capi.WtLoudnessClip * 2)()
        for j, d in enumerate(descs):
            d.x, d.n, d.channels, d.channel_stride, d.out, d.blocks = fake, 9600, 1, 0, fake + 64 + 12 * j, None
        mutate(descs)
        return lib.wt_loudness(descs, B, rate, ctypes.c_void_p(workspace), None)

    def setter(j, field, value):
        return lambda descs: setattr(descs[j], field, value)

    for what, rc in (("B = 0", call(B=0)), ("B = 65536", call(B=65536)), ("rate 7999", call(rate=7999)), ("rate 192001", call(rate=192001)),
                     ("n = 0", call(setter(1, "n", 0))), ("n < 0", call(setter(0, "n", -3))), ("channels 0", call(setter(1, "channels", 0))),
                     ("channels 3", call(setter(0, "channels", 3))), ("null x", call(setter(1, "x", None))),
                     ("misaligned x", call(setter(0, "x", fake + 2))), ("null out", call(setter(1, "out", None))),
                     ("misaligned out", call(setter(1, "out", fake + 65))), ("misaligned blocks", call(setter(0, "blocks", fake + 1))),
                     ("null workspace", call(workspace=None)), ("misaligned workspace", call(workspace=fake + 4))):
        assert rc == INVALID, what
        assert b"wt_loudness" in lib.wt_last_error(), what
    assert lib.wt_loudness(None, 2, 24000, ctypes.c_void_p(fake), None) == INVALID

    def norm(n=(9600, 9600), rows=fake, T_pad=9600, rate=24000, target=-23.0, scales=fake + 64, workspace=fake + 128, B=2):
        return lib.wt_normalize_rows_lufs(ctypes.c_void_p(rows), B, T_pad, (ctypes.c_int64 * 2)(*n), rate, target, ctypes.c_void_p(scales),
                                          ctypes.c_void_p(workspace), None)

    for what, rc in (("n > T_pad", norm(n=(9600, 9601))), ("n = 0", norm(n=(0, 9600))), ("null rows", norm(rows=None)),
                     ("misaligned rows", norm(rows=fake + 2)), ("T_pad = 0", norm(T_pad=0)), ("rate", norm(rate=4000)),
                     ("target nan", norm(target=float("nan"))), ("target inf", norm(target=float("inf"))),
                     ("target -inf", norm(target=-float("inf"))), ("null scales", norm(scales=None)), ("misaligned scales", norm(scales=fake + 66)),
                     ("null workspace", norm(workspace=None)), ("misaligned workspace", norm(workspace=fake + 4)), ("B = 0", norm(B=0))):
        assert rc == INVALID, what
        assert b"wt_normalize_rows_lufs" in lib.wt_last_error(), what


def test_lufs_arguments_raise_before_any_gpu_work(model):
    wav = torch.zeros(1, 12000)
    clips = [torch.zeros(12000)]
    calls = {
        "encode_codes": lambda **kw: model.encode_codes(wav, **kw),
        "encode_codes_many": lambda **kw: model.encode_codes_many(clips, **kw),
        "encode_codes_segmented": lambda **kw: model.encode_codes_segmented(clips[0], 1200, 600, **kw),
        "encode_codes_segmented_many": lambda **kw: model.encode_codes_segmented_many(clips, 1200, 600, **kw),
    }
    for name, call in calls.items():
        for kw in (dict(normalize="lufs", target_db=-3.0), dict(target_lufs=-16.0), dict(normalize="peak", target_lufs=-16.0),
                   dict(normalize="rms", target_lufs=-16.0), dict(target_lufs=-23.0), dict(normalize="peak", target_lufs=-23.0),
                   dict(normalize="rms", target_lufs=-23), dict(normalize="lufs", target_lufs=float("nan")),
                   dict(normalize="lufs", target_lufs=float("inf")), dict(normalize="lufs", target_lufs="-23"),
                   dict(normalize="lufs", target_lufs=[-23.0]), dict(normalize="lufs", target_lufs=True), dict(normalize="loudness"),
                   dict(normalize="LUFS")):
            with pytest.raises(ValueError):
                call(**kw)
        with pytest.raises(RuntimeError):                      # the arguments are fine: the next thing is the GPU
            call(normalize="lufs")
        with pytest.raises(RuntimeError):
            call(normalize="lufs", target_lufs=-16)
        with pytest.raises(RuntimeError):                      # None: not given, the default of -23
            call(normalize="lufs", target_lufs=None)


def test_audio_and_metrics_arguments():
    from wavtokenizer_amd import _capi, audio, metrics
    x = torch.zeros(2, 12000)
    for kw in (dict(mode="loudness"), dict(mode="lufs", target_db=-3.0), dict(mode="peak", target_lufs=-16.0),
               dict(mode="peak", target_lufs=-23.0), dict(mode="rms", target_lufs=-23.0),
               dict(mode="lufs", target_lufs=float("-inf")), dict(mode="lufs", target_lufs=[-23.0]), dict(mode="lufs", sample_rate=7999),
               dict(mode="lufs", sample_rate=24000.0)):
        with pytest.raises(ValueError):
            audio.normalize(x, **kw)
    with pytest.raises(TypeError):                             # the new arguments are keyword-only
        audio.normalize(x, "lufs", 0.0, -16.0)
    with pytest.raises(RuntimeError, match="GPU only"):        # there is no CPU path
        audio.normalize(x, mode="lufs")
    assert audio.normalize_args("f", "lufs", 0.0) == (_capi.WT_NORM_LUFS, -23.0)
    assert audio.normalize_args("f", "lufs", 0, -16) == (_capi.WT_NORM_LUFS, -16.0)
    assert audio.normalize_args("f", "lufs", 0.0, None) == (_capi.WT_NORM_LUFS, -23.0)
    assert audio.normalize_args("f", None, 0.0) is None and audio.normalize_args("f", "rms", 0.0) == (1, 1.0)
    with pytest.raises(ValueError, match="sample_rate"):       # the rows' rate is the caller's to state, never a silent default
        audio.normalize_rows(torch.zeros(1, 12000), [12000], _capi.WT_NORM_LUFS, -23.0)
    clip = torch.zeros(12000)
    for bad in ([], [torch.zeros(0)], [torch.zeros(3, 100)], [torch.zeros(1, 2, 100)], [torch.zeros(100, dtype=torch.float64)], [[0.0]]):
        with pytest.raises(ValueError):
            audio.loudness_many(bad)
    for rate in (7999, 192001, 24000.0, "24000", [24000, 16000], True):
        with pytest.raises(ValueError):
            audio.loudness_many([clip], rate)
    with pytest.raises(RuntimeError, match="GPU only"):
        audio.loudness(clip)
    with pytest.raises(RuntimeError, match="GPU only"):
        audio.loudness_many([clip, torch.zeros(2, 9000)], [24000, 48000], momentary=True)
    for a, b in (([clip], []), ([], []), ([clip], [torch.zeros(3, 100)])):
        with pytest.raises(ValueError):
            metrics.loudness_delta_many(a, b)
    with pytest.raises(ValueError):
        metrics.loudness_delta_many([clip], [clip], sample_rate=[24000, 24000])
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.loudness_delta(clip, clip)


def test_the_reference_reads_the_standards_sine():
    """EBU Tech 3341, case 1 in spirit: a 997 Hz sine at 0 dBFS in one channel reads -3.01 LUFS; in both of two channels at
    -23 dBFS it reads -23.0 LUFS."""
    fs = 48000
    t = np.arange(5 * fs) / fs
    sine = np.sin(2 * np.pi * 997.0 * t)
    L, gamma, count, l = R.loudness(sine, fs)
    assert abs(L + 3.01) <= 0.005 and abs(L + 3.0103) < 2e-4, L
    assert count == len(l) == R.blocks(5 * fs, fs) == 47 and abs(gamma - (L - 10.0)) < 1e-3
    quiet = sine * 10.0 ** (-23.0 / 20.0)
    L2 = R.loudness(np.stack([quiet, quiet]), fs)[0]
    assert abs(L2 + 23.0) <= 0.005 and abs(L2 + 22.99997) < 2e-4, L2
    # silence, and a clip under 400 ms
    assert R.loudness(np.zeros(fs), fs)[:3] == (-math.inf, -math.inf, 0)
    assert R.loudness(sine[:19199], fs)[:3] == (-math.inf, -math.inf, 0) and R.loudness(sine[:19200], fs)[2] == 1
    # the bound: the fp32 evaluation's error, at least two ulps
    assert R.bound(-23.0, -23.0) == 2 * R.ulp32(-23.0) == 2.0 ** -18 and R.bound(-23.0, -23.001) == pytest.approx(0.001)
    assert R.bound(-math.inf, -math.inf) == 0.0


def test_the_chunked_stand_in_is_the_sequential_filter_in_another_order():
    """loudness_ref.weighted_chunked (what bound64 is taken from) against the sequential float64 lfilter: more than 64 groups of
    64 chunks at 192 kHz on content under the high pass, where the carry across groups matters; a short stereo clip; a chunk of 32."""
    from wavtokenizer_amd import _capi
    C = int(_capi.lib.wt_loudness_chunk())
    fs, n = 192000, 65 * 64 * C + 17
    x = R.make_low_clip(n, fs, seed=5)
    y, yc = R.weighted(x, fs), R.weighted_chunked(x, fs, C)
    assert yc.shape == y.shape == (1, n) and yc.dtype == np.float64
    assert np.abs(yc - y).max() <= 1e-7 * np.abs(y).max()
    assert np.abs(yc - y).max() > 0                            # (another order: not the same text run twice)
    L, Lc = R.loudness(x, fs)[0], R.loudness(x, fs, y=yc)[0]
    assert 4.0 * abs(Lc - L) < R.ulp32(L)
    s = np.stack([R.make_clip(3 * C + 5, seed=6), R.make_clip(3 * C + 5, seed=7)])
    for chunk in (C, 32):
        assert np.abs(R.weighted_chunked(s, 8001, chunk) - R.weighted(s, 8001)).max() <= 1e-12
    # bound64: two ulps and four times the stand-in's distance
    assert R.bound64(-23.0, -23.0) == 2.0 ** -18 and R.bound64(-23.0, -23.0 + 1e-7) == pytest.approx(2.0 ** -18 + 4e-7, rel=1e-6)
    assert R.bound64(-math.inf, -math.inf) == 0.0
