"""The host side of decode-from-codes without a GPU: the constants of the two plan kinds, the probe op and its kernel ids on both
sides of the C ABI, and the control flow of WavTokenizer.decode_codes_many over recording stubs."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_capi_constants_agree():
    from wavtokenizer_amd import _capi          # (binds the built library: the entry points must be exported)
    with open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")) as f:
        h = f.read()

    def const(name):
        return int(re.search(r"\b%s\s*=\s*(\d+)" % name, h).group(1))

    assert const("WT_PLAN_DECODE_CODES") == _capi.WT_PLAN_DECODE_CODES == 6
    assert const("WT_PLAN_DECODE_CODES_MIXED") == _capi.WT_PLAN_DECODE_CODES_MIXED == 7
    assert const("WT_OP_CODE_ROWS") == _capi.WT_OP_CODE_ROWS
    # op id 11 stays unassigned: tests/test_op_checks.py probes it as the first id the library does not know, with a
    # descriptor of stand-in pointers that a CODE_ROWS launch would read
    assert _capi.WT_OP_CODE_ROWS == 12 and not re.search(r"\bWT_OP_\w+\s*=\s*11\b", h)
    assert const("WT_OPK_CODE_ROWS") == _capi.WT_OPK_CODE_ROWS == 22 and _capi.WT_OPK_NAMES[22] == "code_rows"
    assert const("WT_OPK_CODE_ROWS_MIXED") == _capi.WT_OPK_CODE_ROWS_MIXED == 23 and _capi.WT_OPK_NAMES[23] == "code_rows_mixed"
    for name, nargs in (("wt_decode_codes", 8), ("wt_decode_codes_mixed", 8)):
        assert name in _capi.EXPORTS and re.search(r"\bint %s\(" % name, h)
        fn = getattr(_capi.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    # the descriptor is the one every existing caller fills
    assert _capi.WtOpDesc._fields_[-1][0] == "lengths"


def test_probe_refuses_code_rows_descriptors_before_any_hip_call():
    """C % 4, S32 with C % 32, K < 1, bins < 1, null arrays: WT_ERR_INVALID with a message; the pointers are not even valid."""
    import ctypes
    from wavtokenizer_amd import _capi
    fake = 1 << 20

    def rc(**kw):
        d = _capi.WtOpDesc()
        d.size = ctypes.sizeof(d)
        d.op, d.B, d.L, d.C, d.k, d.n = _capi.WT_OP_CODE_ROWS, 3, 5, 64, 3, 7
        d.x, d.p0, d.y = fake, 2 * fake, 3 * fake
        for k, v in kw.items():
            setattr(d, k, v)
        return _capi.lib.wt_op_probe(ctypes.byref(d), None, None), _capi.lib.wt_last_error().decode()

    for kw, msg in ((dict(C=30), "C % 4"), (dict(C=36, out_s32=1), "C % 32"), (dict(k=0), "k >= 1"), (dict(n=0), "bins"),
                    (dict(x=None), "x missing"), (dict(p0=None), "null"), (dict(y=None), "null"), (dict(C=1028), "C <= 1024"),
                    (dict(B=0), "positive"), (dict(lengths=fake + 2), "lengths misaligned")):
        code, err = rc(**kw)
        assert code == _capi.WT_ERR_INVALID and msg in err, (kw, err)


# ----------------------------------------------------------------------------------------- decode_codes_many on stubs
class _Recorder:
    """Stands in for _run_decode_codes_mixed and decode_codes on a model that was never loaded: records what it is sent."""

    def __init__(self, model, refuse=()):
        self.m, self.refuse = model, set(refuse)
        self.mixed, self.solo = [], []

    def run_mixed(self, codes_list, L_pad, bw, dev=None):
        lengths = [int(c.shape[1]) for c in codes_list]
        assert len(codes_list) >= 2 and max(lengths) <= L_pad and all(c.dim() == 2 for c in codes_list)
        self.mixed.append((L_pad, lengths, bw))
        if L_pad in self.refuse:
            return None                                      # off route: the caller takes these clips one at a time
        wav = torch.zeros((len(codes_list), self.m._wave_len(L_pad)))
        for j, L in enumerate(lengths):
            wav[j, :self.m._wave_len(L)] = float(L)          # clip j carries its own length, zeros behind it
        return wav

    def decode_codes(self, codes, bandwidth_id=None):
        assert codes.dim() == 2
        L = int(codes.shape[1])
        self.solo.append((L, bandwidth_id))
        return torch.full((1, self.m._wave_len(L)), float(L))


def _stubbed(refuse=()):
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(ARCH_HOP600)                  # on the CPU, no engine: any real call would raise
    rec = _Recorder(m, refuse)
    m._run_decode_codes_mixed = rec.run_mixed
    m.decode_codes = rec.decode_codes
    return m, rec


def _clip(L, K=1, dtype=torch.int64):
    return torch.zeros((K, L), dtype=dtype)


def test_decode_codes_many_validates_its_inputs():
    m, rec = _stubbed()
    for bad in ([torch.zeros(5, dtype=torch.int64)],                      # wrong rank
                [torch.zeros((1, 2, 5), dtype=torch.int64)],              # (K, B, L) with B != 1
                [_clip(5), _clip(7, K=2)],                                # K differs (and exceeds the model's codebooks)
                [_clip(0)],                                               # L = 0
                [_clip(5, dtype=torch.float32)],                          # codes are integers
                [_clip(5, dtype=torch.bool)],
                [[1, 2, 3]]):                                             # not a tensor
        with pytest.raises(ValueError):
            m.decode_codes_many(bad, bandwidth_id=0)
    assert not rec.mixed and not rec.solo
    assert m.decode_codes_many([], bandwidth_id=0) == []


def test_mixed_k_is_refused_on_a_model_with_several_codebooks():
    import dataclasses
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(dataclasses.replace(ARCH_HOP600, num_quantizers=3))
    rec = _Recorder(m)
    m._run_decode_codes_mixed, m.decode_codes = rec.run_mixed, rec.decode_codes
    with pytest.raises(ValueError, match="same K"):
        m.decode_codes_many([_clip(5, K=2), _clip(7, K=3)], bandwidth_id=0)
    with pytest.raises(ValueError, match="same K"):
        m.decode_codes_many([_clip(5, K=4)], bandwidth_id=0)
    out = m.decode_codes_many([_clip(5, K=3), _clip(6, K=3)], bandwidth_id=0)
    assert [tuple(o.shape) for o in out] == [(1, 5 * 600), (1, 6 * 600)] and rec.mixed == [(6, [5, 6], 0)]


def test_decode_codes_many_sends_every_clip_once_and_in_order():
    from wavtokenizer_amd.mixed_length import group_frames
    m, rec = _stubbed()
    frames = [200, 1, 256, 3, 2, 7, 300, 31, 33, 32, 129, 128, 127, 255, 257, 12000, 400, 384, 385]
    clips = [_clip(L) if i % 2 else _clip(L)[:, None, :] for i, L in enumerate(frames)]
    out = m.decode_codes_many(clips, bandwidth_id=torch.tensor([2]))
    assert len(out) == len(frames)
    for L, o in zip(frames, out):                            # input order, each clip's own samples
        assert o.shape == (1, m._wave_len(L)) and bool((o == float(L)).all())
    groups = group_frames(frames)                            # decode_many's groups and buckets
    want_mixed = [(L_pad, [frames[i] for i in idx], 2) for L_pad, idx in groups if len(idx) > 1]
    want_solo = sorted(i for _L_pad, idx in groups if len(idx) == 1 for i in idx)
    assert rec.mixed == want_mixed
    assert [L for L, _bw in rec.solo] == [frames[i] for i in want_solo] and 12000 in [L for L, _bw in rec.solo]
    assert all(bw == 2 for _L, bw in rec.solo)
    sent = sorted([L for _p, ls, _b in rec.mixed for L in ls] + [L for L, _b in rec.solo])
    assert sent == sorted(frames)                            # every clip exactly once


def test_none_from_the_mixed_call_goes_to_the_solo_path():
    from wavtokenizer_amd.mixed_length import group_frames
    frames = [5, 6, 7, 100, 101, 102]
    groups = group_frames(frames)
    assert len(groups) == 2 and all(len(idx) == 3 for _L, idx in groups)
    refused = groups[0][0]
    m, rec = _stubbed(refuse=[refused])
    out = m.decode_codes_many([_clip(L) for L in frames], bandwidth_id=1)
    assert [int(o[0, 0]) for o in out] == frames
    assert [p for p, _ls, _b in rec.mixed] == [g[0] for g in groups]          # both groups were tried
    assert [L for L, _bw in rec.solo] == [5, 6, 7]                            # the refused group, clip by clip, in order


def test_center_padding_sends_one_frame_clips_alone():
    import dataclasses
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
    m = WavTokenizer.from_arch(dataclasses.replace(ARCH_HOP600, padding="center"))
    rec = _Recorder(m)
    m._run_decode_codes_mixed, m.decode_codes = rec.run_mixed, rec.decode_codes
    m.decode_codes_many([_clip(2), _clip(3), _clip(2)], bandwidth_id=0)
    assert rec.mixed == [(3, [2, 2, 3], 0)] and not rec.solo
    rec.mixed.clear()
    m.decode_codes_many([_clip(3), _clip(1), _clip(2)], bandwidth_id=0)      # a group that starts below two frames (decode raises there)
    assert not rec.mixed and [L for L, _bw in rec.solo] == [3, 1, 2]
