"""The host side of tokenising from PCM without a GPU: the new exports on both sides of the C ABI, wt_ingest's refusals (made
before any device call, with pointers that are not even valid), the argument checks of WavTokenizer.encode_codes_many and its
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
    for name, ret, nargs in (("wt_ingest", "int", 6), ("wt_codes_unpack", "int", 7), ("wt_ingest_workspace_bytes", "size_t", 1)):
        assert name in _capi.EXPORTS
        decl = re.search(r"\b%s\s+%s\(([^;]*?)\);" % (ret, name), h, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        fn = getattr(_capi.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    assert int(re.search(r"\bWT_INGEST_F32\s*=\s*(\d+)", h).group(1)) == _capi.WT_INGEST_F32 == 0
    assert int(re.search(r"\bWT_INGEST_I16\s*=\s*(\d+)", h).group(1)) == _capi.WT_INGEST_I16 == 1
    # the descriptor's fields, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} wt_ingest_clip;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            fields += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
    assert fields == [f[0] for f in _capi.WtIngestClip._fields_], fields
    assert ctypes.sizeof(_capi.WtIngestClip) == 56
    assert _capi.lib.wt_ingest_workspace_bytes(64) >= 64 * 56 and _capi.lib.wt_ingest_workspace_bytes(0) == 0
    # op id 11 of the probe stays unassigned (tests/test_op_checks.py relies on it)
    assert not re.search(r"\bWT_OP_\w+\s*=\s*11\b", h)
    assert "features may be NULL" in h or "may be NULL (a caller that wants the codes alone" in h


class _FakeResampler(ctypes.Structure):
    """The library's wt_resampler (csrc/audio.hip): device, the gcd-reduced rates, taps per phase, half width, the phase table.
    The table pointer stays null here: a launch would read it, a refusal must not."""
    _fields_ = [("device", ctypes.c_int), ("orig", ctypes.c_int), ("nw", ctypes.c_int), ("K", ctypes.c_int), ("width", ctypes.c_int),
                ("kern", ctypes.c_void_p)]


def test_ingest_refuses_bad_descriptors_before_any_hip_call():
    from wavtokenizer_amd import _capi
    from wavtokenizer_amd.audio import resampler_geometry
    fake = 1 << 20                                           # not a valid address: nothing may be dereferenced
    orig, nw, width, K = resampler_geometry(44100, 24000)
    r0 = _FakeResampler(0, orig, nw, K, width, None)
    r1 = _FakeResampler(1, orig, nw, K, width, None)        # the same pair on another device
    n_in = 1000
    n_out = -(-nw * n_in // orig)
    assert _capi.lib.wt_resampler_out_length(ctypes.addressof(r0), n_in) == n_out

    def rc(second=None, T_pad=4096, out=fake * 3, ws=fake * 4, **kw):
        clips = (_capi.WtIngestClip * 2)()
        for c in clips:
            c.src, c.dtype, c.channels, c.n_in, c.ch_stride, c.sample_stride = fake, _capi.WT_INGEST_I16, 2, n_in, 1, 2
            c.resampler, c.n_out = ctypes.addressof(r0), n_out
        for k, v in (second or kw).items():
            setattr(clips[1 if second else 0], k, v)
        return _capi.lib.wt_ingest(clips, 2, T_pad, out, ws, None), _capi.lib.wt_last_error().decode()

    cases = [(dict(src=None), "null source"), (dict(channels=3), "mono or stereo"), (dict(channels=0), "mono or stereo"),
             (dict(n_in=0), "n_in < 1"), (dict(n_out=n_out + 1), "wt_resampler_out_length"),
             (dict(n_out=n_out - 1), "wt_resampler_out_length"), (dict(src=fake + 1), "misaligned"),
             (dict(src=fake + 2, dtype=_capi.WT_INGEST_F32), "misaligned"), (dict(dtype=2), "fp32 or int16"),
             (dict(resampler=None), "null resampler"), (dict(sample_stride=-1), "negative stride")]
    for kw, msg in cases:
        for second in (None, kw):                            # as the first clip of the call and behind a good one
            code, err = rc(second=second, **({} if second else kw))
            assert code == _capi.WT_ERR_INVALID and msg in err, (kw, err)
    code, err = rc(T_pad=n_out - 1)
    assert code == _capi.WT_ERR_INVALID and "n_out > T_pad" in err
    code, err = rc(second=dict(resampler=ctypes.addressof(r1)))
    assert code == _capi.WT_ERR_INVALID and "another device" in err
    for kw in (dict(out=None), dict(ws=None), dict(T_pad=0)):
        code, err = rc(**kw)
        assert code == _capi.WT_ERR_INVALID and "bad argument" in err, kw
    assert _capi.lib.wt_ingest(None, 2, 4096, fake, fake, None) == _capi.WT_ERR_INVALID
    assert _capi.lib.wt_codes_unpack(None, 1, 8, fake, fake, 8, None) == _capi.WT_ERR_INVALID
    assert _capi.lib.wt_codes_unpack(fake, 1, 8, fake + 4, fake, 8, None) == _capi.WT_ERR_INVALID
    assert _capi.lib.wt_codes_unpack(fake, 0, 8, fake, fake, 8, None) == _capi.WT_ERR_INVALID


def test_resampler_geometry_matches_the_length_rule():
    from wavtokenizer_amd.audio import resampled_length, resampler_geometry
    assert resampler_geometry(24000, 24000) == (1, 1, 0, 1)
    assert resampler_geometry(44100, 24000) == (147, 80, 12, 171)
    assert resampler_geometry(11025, 24000)[:2] == (147, 320)
    for sr in (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000):
        for T in (1, 255, 7001, 30011):
            assert resampled_length(sr, 24000, T) == math.ceil(24000 * T / sr)
    for bad in ((0, 24000), (-1, 24000), (7999, 24000)):     # (7999 and 24000 are coprime: 8013 taps per phase)
        with pytest.raises(ValueError):
            resampler_geometry(*bad)


# --------------------------------------------------------------------------------------- encode_codes_many on stubs
class _Recorder:
    """Stands in for _run_encode_codes_mixed and _encode_codes_solo on a model that was never loaded: records what it is sent
    and writes each clip's index + 1 over the clip's span of the flat tensor."""

    def __init__(self, refuse=()):
        self.refuse = set(refuse)
        self.mixed, self.solo, self.tag, self.seen = [], [], {}, set()

    def run_mixed(self, specs, T_pad, flat, offsets):
        assert all(1024 <= sp.n_out <= T_pad for sp in specs) and len(specs) <= 64
        self.mixed.append((T_pad, [sp.n_out for sp in specs]))
        if T_pad in self.refuse:
            return None                                      # off route: the caller takes these clips one at a time
        self._write(specs, flat, offsets)
        return True

    def run_solo(self, specs, flat, offsets):
        self.solo.append([sp.n_out for sp in specs])
        self._write(specs, flat, offsets)

    def _write(self, specs, flat, offsets):
        for sp, off in zip(specs, offsets):
            L = -(-sp.n_out // 600)
            assert id(sp.clip) not in self.seen, "a clip was sent twice"
            self.seen.add(id(sp.clip))
            flat[off:off + L] = self.tag[id(sp.clip)]


def _stubbed(refuse=()):
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(ARCH_HOP600)                  # on the CPU, no engine: any real call would raise
    rec = _Recorder(refuse)
    m._run_encode_codes_mixed, m._encode_codes_solo = rec.run_mixed, rec.run_solo
    return m, rec


def _run(m, rec, clips, **kw):
    rec.tag = {id(c): i + 1 for i, c in enumerate(clips)}
    return m.encode_codes_many(clips, **kw)


def test_encode_codes_many_validates_its_arguments():
    m, rec = _stubbed()
    f = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    for bad, kw in (([f(2, 3, 2000)], {}),                               # wrong rank
                    ([torch.tensor(1.0)], {}),
                    ([f(3, 2000)], {}),                                  # three channels
                    ([f(2000, 2)], {}),                                  # (T, C) without channels_last: 2000 channels
                    ([f(2, 2000)], dict(channels_last=True)),            # (C, T) with channels_last
                    ([f(0, 2000)], {}),
                    ([f(2000, dtype=torch.float64)], {}),                # wrong dtype
                    ([f(2000, dtype=torch.int32)], {}),
                    ([f(0)], {}), ([f(2, 0)], {}), ([f(0, 1)], dict(channels_last=True)),      # empty
                    ([f(2000), f(2000)], dict(sample_rates=[24000])),    # rate count
                    ([f(2000)], dict(sample_rates=[24000, 16000])),
                    ([f(2000)], dict(sample_rates=0)),
                    ([f(2000)], dict(sample_rates=[7999])),              # a ratio the resampler refuses
                    ([[0.0, 1.0]], {})):                                 # not a tensor
        with pytest.raises(ValueError):
            m.encode_codes_many(bad, **kw)
    assert not rec.mixed and not rec.solo
    assert m.encode_codes_many([]) == []
    flat, offs = m.encode_codes_many([], packed=True)
    assert flat.numel() == 0 and offs.tolist() == [0]


def test_every_clip_is_sent_once_and_offsets_are_the_prefix_sums():
    from wavtokenizer_amd.mixed_length import group_clips
    m, rec = _stubbed()
    rates = [16000, 22050, 24000, 44100, 48000, 11025, 8000, 32000, 24000, 48000, 16000, 44100]
    T = [9000, 7001, 5000, 30011, 2049, 4000, 350, 1, 1023, 2046, 72000, 441000]
    clips = []
    for i, t in enumerate(T):
        dt = torch.int16 if i % 2 else torch.float32
        clips.append([torch.zeros(t, dtype=dt), torch.zeros((2, t), dtype=dt), torch.zeros((1, t), dtype=dt)][i % 3])
    n_out = [math.ceil(24000 * t / sr) for t, sr in zip(T, rates)]
    frames = [m.arch.frames(n) for n in n_out]
    flat, offs = _run(m, rec, clips, sample_rates=rates, packed=True)
    assert offs.device.type == "cpu" and offs.dtype == torch.int64
    assert offs.tolist() == [sum(frames[:i]) for i in range(len(T) + 1)] and flat.shape == (sum(frames),) and flat.dtype == torch.int64
    for i in range(len(T)):                                  # every span was written, by its own clip
        assert bool((flat[offs[i]:offs[i + 1]] == i + 1).all()), i
    groups, solo = group_clips(n_out, 600)
    assert rec.mixed == [(T_pad, [n_out[i] for i in idx]) for T_pad, idx in groups]
    assert rec.solo == [[n_out[i] for i in sorted(solo)]]
    assert sorted(n_out[i] for i in solo) == sorted(n for n in n_out if n < 1024) and len(solo) == 3   # 1 @ 32 k, 1023, 2046 @ 48 k
    sent = sorted([n for _p, ns in rec.mixed for n in ns] + [n for ns in rec.solo for n in ns])
    assert sent == sorted(n_out)
    # the list form: views into the one flat tensor, in input order
    m2, rec2 = _stubbed()
    out = _run(m2, rec2, clips, sample_rates=rates)
    assert [tuple(o.shape) for o in out] == [(1, 1, L) for L in frames]
    assert all(bool((o == i + 1).all()) for i, o in enumerate(out))
    base = out[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == base for o in out)
    # channels_last and one rate for every clip; the default rate is the codec's
    m3, rec3 = _stubbed()
    out = _run(m3, rec3, [torch.zeros((4410, 2), dtype=torch.int16), torch.zeros((8820, 1))], sample_rates=44100, channels_last=True)
    assert [o.shape[-1] for o in out] == [4, 8] and rec3.mixed == [(4800, [2400, 4800])]
    m4, rec4 = _stubbed()
    out = _run(m4, rec4, [torch.zeros(2400), torch.zeros(1200)])
    assert [o.shape[-1] for o in out] == [4, 2] and rec4.mixed == [(2400, [1200, 2400])]


def test_none_from_the_mixed_call_goes_to_the_solo_path():
    from wavtokenizer_amd.mixed_length import group_clips
    T = [2000, 2100, 2200, 40000, 41000, 42000, 500]
    groups, solo = group_clips(T, 600)
    assert len(groups) == 2 and solo == [6]
    m, rec = _stubbed(refuse=[groups[0][0]])
    clips = [torch.zeros(t) for t in T]
    out = _run(m, rec, clips)
    assert [int(o[0, 0, 0]) for o in out] == list(range(1, len(T) + 1))
    assert [p for p, _ns in rec.mixed] == [g[0] for g in groups]              # both groups were tried
    assert rec.solo == [[2000, 2100, 2200, 500]]                              # the refused group and the short clip, in input order
