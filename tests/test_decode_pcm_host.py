"""The host side of synthesising to PCM without a GPU: the new exports on both sides of the C ABI, wt_emit's refusals (made
before any device call, with pointers that are not even valid), the argument checks of WavTokenizer.decode_pcm_many and its
control flow over recording stubs."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_capi_agree_on_the_new_exports():
    from wavtokenizer_amd import _capi          # (binds the built library: the entry points must be exported)
    with open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")) as f:
        h = f.read()
    for name, ret, nargs in (("wt_emit", "int", 4), ("wt_emit_workspace_bytes", "size_t", 1)):
        assert name in _capi.EXPORTS
        decl = re.search(r"\b%s\s+%s\(([^;]*?)\);" % (ret, name), h, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        fn = getattr(_capi.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    assert "WtEmitClip" in dir(_capi)
    assert int(re.search(r"\bWT_EMIT_F32\s*=\s*(\d+)", h).group(1)) == _capi.WT_EMIT_F32 == 0
    assert int(re.search(r"\bWT_EMIT_I16\s*=\s*(\d+)", h).group(1)) == _capi.WT_EMIT_I16 == 1
    # the descriptor's fields, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} wt_emit_clip;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            fields += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
    assert fields == [f[0] for f in _capi.WtEmitClip._fields_], fields
    assert fields == ["src", "n_in", "resampler", "n_out", "dst", "dtype", "channels", "ch_stride", "sample_stride", "limit"]
    assert ctypes.sizeof(_capi.WtEmitClip) == 72
    doc = h[h.index("Ragged emit"):h.index("wt_emit_dtype")]
    assert "must NOT be called on a stream that" in doc and "captured into a graph" in doc


def test_workspace_size_grows_with_the_clips():
    from wavtokenizer_amd import _capi
    ws = _capi.lib.wt_emit_workspace_bytes
    assert ws(0) == 0 and ws(-3) == 0
    assert 0 < ws(1) < ws(2) < ws(64) and ws(64) == 64 * ws(1) and ws(1) % 8 == 0


class _FakeResampler(ctypes.Structure):
    """The library's wt_resampler (csrc/audio.hip): device, the gcd-reduced rates, taps per phase, half width, the phase table.
    The table pointer stays null here: a launch would read it, a refusal must not."""
    _fields_ = [("device", ctypes.c_int), ("orig", ctypes.c_int), ("nw", ctypes.c_int), ("K", ctypes.c_int), ("width", ctypes.c_int),
                ("kern", ctypes.c_void_p)]


def test_emit_refuses_bad_descriptors_before_any_hip_call():
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.audio import resampler_geometry
    fake = 1 << 20                                           # not a valid address: nothing may be dereferenced
    orig, nw, width, K = resampler_geometry(24000, 44100)
    r0 = _FakeResampler(0, orig, nw, K, width, None)
    r1 = _FakeResampler(1, orig, nw, K, width, None)        # the same pair on another device
    # a pair wt_resampler_create itself refuses: its window (256 / nw + 2) * orig + K floats is beyond 64 KiB
    wide = _FakeResampler(0, 24000, 7999, 2 * 19 + 24000, 19, None)
    n_in = 1000
    n_out = -(-nw * n_in // orig)
    assert _capi.lib.wt_resampler_out_length(ctypes.addressof(r0), n_in) == n_out

    def rc(second=None, ws=fake * 4, **kw):
        clips = (_capi.WtEmitClip * 2)()
        for c in clips:
            c.src, c.n_in, c.resampler, c.n_out, c.dst = fake, n_in, ctypes.addressof(r0), n_out, fake * 2
            c.dtype, c.channels, c.ch_stride, c.sample_stride, c.limit = _capi.WT_EMIT_I16, 2, 1, 2, 0.99
        for k, v in kw.items():
            setattr(clips[0], k, v)
        for k, v in (second or {}).items():
            setattr(clips[1], k, v)
        return _capi.lib.wt_emit(clips, 2, ws, None), _capi.lib.wt_last_error().decode()

    wide_out = _capi.lib.wt_resampler_out_length(ctypes.addressof(wide), n_in)
    cases = [(dict(src=None), "null source"), (dict(dst=None), "null destination"), (dict(resampler=None), "null resampler"),
             (dict(dtype=2), "fp32 or int16"), (dict(dtype=-1), "fp32 or int16"),
             (dict(channels=3), "channels must be 1 or 2"), (dict(channels=0), "channels must be 1 or 2"),
             (dict(n_in=0), "n_in < 1"), (dict(n_out=n_out + 1), "wt_resampler_out_length"),
             (dict(n_out=n_out - 1), "wt_resampler_out_length"),
             (dict(ch_stride=-1), "negative stride"), (dict(sample_stride=-2), "negative stride"),
             (dict(ch_stride=0, sample_stride=1), "overlap"), (dict(ch_stride=0, sample_stride=0), "overlap"),
             (dict(ch_stride=1, sample_stride=1), "overlap"), (dict(ch_stride=n_out - 1, sample_stride=1), "overlap"),
             (dict(dst=fake * 2 + 1), "misaligned destination"),
             (dict(dst=fake * 2 + 2, dtype=_capi.WT_EMIT_F32), "misaligned destination"),
             (dict(src=fake + 2), "misaligned source"),
             (dict(limit=0.0), "limit outside (0, 1]"), (dict(limit=1.5), "limit outside (0, 1]"),
             (dict(limit=-0.5), "limit outside (0, 1]"), (dict(limit=float("nan")), "limit outside (0, 1]"),
             (dict(resampler=ctypes.addressof(wide), n_out=wide_out), "LDS window")]
    for kw, msg in cases:
        for second in (None, kw):                            # as the first clip of the call and behind a good one
            code, err = rc(second=second, **({} if second else kw))
            assert code == _capi.WT_ERR_INVALID and msg in err, (kw, err)
    code, err = rc(second=dict(resampler=ctypes.addressof(r1)))
    assert code == _capi.WT_ERR_INVALID and "another device" in err
    code, err = rc(ws=None)
    assert code == _capi.WT_ERR_INVALID and "bad argument" in err
    code, err = rc(ws=fake * 4 + 4)
    assert code == _capi.WT_ERR_INVALID and "misaligned" in err
    assert _capi.lib.wt_emit(None, 2, fake, None) == _capi.WT_ERR_INVALID
    clips = (_capi.WtEmitClip * 1)()
    assert _capi.lib.wt_emit(clips, 0, fake, None) == _capi.WT_ERR_INVALID
    # what is NOT refused: the limit of an fp32 clip is not looked at, ch_stride 0 is a mono clip's, stereo on one slot per
    # frame is fine from sample_stride 2 on, and planar channels may touch (ch_stride = n_out) -- shown by the refusal that comes next in the order of the checks
    for kw in (dict(dtype=_capi.WT_EMIT_F32, dst=fake * 2, limit=0.0), dict(channels=1, ch_stride=0, sample_stride=1),
               dict(ch_stride=0, sample_stride=2), dict(ch_stride=n_out, sample_stride=1)):
        code, err = rc(second=dict(resampler=ctypes.addressof(r1)), **kw)
        assert code == _capi.WT_ERR_INVALID and "clip 1: resampler of another device" in err, (kw, err)


# --------------------------------------------------------------------------------------- decode_pcm_many on stubs
class _Recorder:
    """Stands in for _run_decode_pcm_mixed and _decode_pcm_solo on a model that was never loaded: records what it is sent and
    writes each clip's index + 1 over the clip's span of the flat tensor."""

    def __init__(self, refuse=()):
        self.refuse = set(refuse)
        self.mixed, self.solo, self.tag, self.seen, self.fmt, self.spans = [], [], {}, set(), None, []

    def run_mixed(self, specs, L_pad, bw, flat, offsets, fmt, channels_last):
        assert all(1 <= sp.frames <= L_pad for sp in specs) and 2 <= len(specs) <= 64
        self.mixed.append((L_pad, [sp.frames for sp in specs]))
        if L_pad in self.refuse:
            return None                                      # off route: the caller takes these clips one at a time
        self._write(specs, flat, offsets, fmt)
        return True

    def run_solo(self, specs, bw, flat, offsets, fmt, channels_last):
        self.solo.append([sp.frames for sp in specs])
        self._write(specs, flat, offsets, fmt)

    def _write(self, specs, flat, offsets, fmt):
        self.fmt = fmt
        assert flat.dtype == fmt[0]
        for sp, off in zip(specs, offsets):
            assert sp.codes.data_ptr() not in self.seen, "a clip was emitted twice"
            self.seen.add(sp.codes.data_ptr())
            end = off + sp.n_out * sp.channels
            assert 0 <= off <= end <= flat.numel() and all(end <= a or b <= off for a, b in self.spans), "spans overlap"
            self.spans.append((off, end))
            flat[off:end] = self.tag[sp.codes.data_ptr()]


def _stubbed(refuse=(), arch=None):
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(arch or ARCH_HOP600)          # on the CPU, no engine: any real call would raise
    rec = _Recorder(refuse)
    m._run_decode_pcm_mixed, m._decode_pcm_solo = rec.run_mixed, rec.run_solo
    return m, rec


def _run(m, rec, clips, **kw):
    rec.tag = {c.data_ptr(): i + 1 for i, c in enumerate(clips)}
    return m.decode_pcm_many(clips, bandwidth_id=0, **kw)


def _codes(L, K=1):
    return torch.zeros((K, L), dtype=torch.int64)


def test_decode_pcm_many_validates_its_arguments():
    m, rec = _stubbed()
    good = [_codes(5), _codes(9)]
    for bad, kw in (([torch.zeros((1, 5))], {}),                                  # floating-point codes
                    ([torch.zeros((1, 5), dtype=torch.bool)], {}),
                    ([torch.zeros(5, dtype=torch.int64)], {}),                    # wrong rank
                    ([torch.zeros((1, 2, 5), dtype=torch.int64)], {}),            # (K, B, L) with B != 1
                    ([_codes(0)], {}),                                            # no frames
                    ([_codes(5), _codes(5, K=2)], {}),                            # another K
                    ([_codes(5, K=2)], {}),                                       # more code rows than codebooks
                    ([[1, 2, 3]], {}),                                            # not a tensor
                    (good, dict(dtype=torch.float64)), (good, dict(dtype=torch.int32)), (good, dict(dtype=torch.float16)),
                    (good, dict(channels=0)), (good, dict(channels=3)), (good, dict(channels=True)),
                    (good, dict(channels=[1])), (good, dict(channels=[1, 3])), (good, dict(channels=[1, 2, 1])),
                    (good, dict(limit=0.0)), (good, dict(limit=1.01)), (good, dict(limit=-1.0)), (good, dict(limit=float("nan"))),
                    (good, dict(sample_rates=[24000])), (good, dict(sample_rates=[24000, 16000, 8000])),
                    (good, dict(sample_rates=0)), (good, dict(sample_rates=[16000, -1])),
                    (good, dict(device="meta")),
                    (good, dict(sample_rates=7999))):                             # a ratio the resampler refuses
        with pytest.raises(ValueError):
            m.decode_pcm_many(bad, bandwidth_id=0, **kw)
    with pytest.raises(ValueError):
        m.decode_pcm(_codes(5), sample_rate=7999, bandwidth_id=0)
    with pytest.raises(ValueError):
        m.decode_pcm(_codes(5), dtype=torch.float64, bandwidth_id=0)
    with pytest.raises(ValueError):
        m.decode_pcm(_codes(5), channels=4, bandwidth_id=0)
    with pytest.raises(ValueError):
        m.decode_pcm(_codes(5), channels=[1], bandwidth_id=0)
    with pytest.raises(ValueError):
        m.decode_pcm(_codes(5), limit=2.0, bandwidth_id=0)
    assert not rec.mixed and not rec.solo
    assert m.decode_pcm_many([], bandwidth_id=0) == []
    flat, offs = m.decode_pcm_many([], packed=True, dtype=torch.float32, bandwidth_id=0)
    assert flat.numel() == 0 and flat.dtype == torch.float32 and offs.tolist() == [0]


def test_every_clip_is_emitted_once_and_offsets_are_the_prefix_sums():
    from wavtokenizer_amd.mixed_length import group_frames
    m, rec = _stubbed()
    L = [1, 2, 3, 7, 40, 41, 75, 1, 300, 9, 9, 160]
    rates = [8000, 16000, 22050, 24000, 44100, 48000] * 2
    clips = [_codes(l) for l in L]
    n_out = [math.ceil(r * 600 * l / 24000) for r, l in zip(rates, L)]
    flat, offs = _run(m, rec, clips, sample_rates=rates, channels=2, channels_last=True, packed=True)
    assert offs.device.type == "cpu" and offs.dtype == torch.int64
    assert offs.tolist() == [2 * sum(n_out[:i]) for i in range(len(L) + 1)]
    assert flat.shape == (2 * sum(n_out),) and flat.dtype == torch.int16 and rec.fmt == (torch.int16, 0.99)
    for i in range(len(L)):                                  # every span was written, by its own clip
        assert bool((flat[offs[i]:offs[i + 1]] == i + 1).all()), i
    groups = group_frames(L)
    assert rec.mixed == [(L_pad, [L[i] for i in idx]) for L_pad, idx in groups if len(idx) > 1]
    lone = sorted(i for _p, idx in groups if len(idx) == 1 for i in idx)
    assert rec.solo == ([[L[i] for i in lone]] if lone else [])
    sent = sorted([n for _p, ns in rec.mixed for n in ns] + [n for ns in rec.solo for n in ns])
    assert sent == sorted(L)
    # the list form: views into the one flat tensor, in input order, in both layouts; one rate for all; the codec rate by default
    for kw, shape in ((dict(channels=2, channels_last=True), lambda n: (n, 2)), (dict(channels=2), lambda n: (2, n)),
                      (dict(dtype=torch.float32), lambda n: (1, n)), (dict(dtype=torch.float32, channels_last=True), lambda n: (n, 1))):
        m2, rec2 = _stubbed()
        out = _run(m2, rec2, clips, sample_rates=rates, **kw)
        assert [tuple(o.shape) for o in out] == [shape(n) for n in n_out], kw
        assert all(bool((o == i + 1).all()) for i, o in enumerate(out))
        base = out[0].untyped_storage().data_ptr()
        assert all(o.untyped_storage().data_ptr() == base for o in out)
        assert out[0].dtype == kw.get("dtype", torch.int16)
    m3, rec3 = _stubbed()
    out = _run(m3, rec3, [_codes(4), _codes(5, K=1)[:, None, :]], sample_rates=48000)
    assert [tuple(o.shape) for o in out] == [(1, 4800), (1, 6000)]
    m4, rec4 = _stubbed()
    out = _run(m4, rec4, [_codes(4), _codes(5)])
    assert [tuple(o.shape) for o in out] == [(1, 2400), (1, 3000)]
    # a channel count per clip: the offsets follow n_out_i * channels_i
    m5, rec5 = _stubbed()
    chans = [1 + i % 2 for i in range(len(L))]
    flat, offs = _run(m5, rec5, clips, sample_rates=rates, channels=chans, channels_last=True, packed=True)
    assert offs.tolist() == [sum(n * c for n, c in zip(n_out[:i], chans[:i])) for i in range(len(L) + 1)]
    assert all(bool((flat[offs[i]:offs[i + 1]] == i + 1).all()) for i in range(len(L)))


def test_none_from_the_mixed_call_goes_to_the_solo_path():
    from wavtokenizer_amd.mixed_length import group_frames
    L = [3, 4, 4, 70, 75, 80, 1000]
    groups = group_frames(L)
    assert [idx for _p, idx in groups] == [[0, 1, 2], [3, 4, 5], [6]]
    m, rec = _stubbed(refuse=[groups[0][0]])
    clips = [_codes(l) for l in L]
    out = _run(m, rec, clips)
    assert [int(o[0, 0]) for o in out] == list(range(1, len(L) + 1))
    assert [p for p, _ns in rec.mixed] == [groups[0][0], groups[1][0]]         # both groups were tried
    assert rec.solo == [[3, 4, 4, 1000]]                                       # the refused group and the lone clip, in input order


def test_center_clips_under_two_frames_go_solo():
    import dataclasses
    from wavtokenizer_amd import ARCH_HOP600
    m, rec = _stubbed(arch=dataclasses.replace(ARCH_HOP600, padding="center"))
    L = [1, 1, 5, 6]
    out = _run(m, rec, [_codes(l) for l in L], sample_rates=48000)
    assert [tuple(o.shape) for o in out] == [(1, 0), (1, 0), (1, 4800), (1, 6000)]      # wave_len = (L - 1) * hop
    assert rec.solo == [[1, 1]] and [ns for _p, ns in rec.mixed] == [[5, 6]]
