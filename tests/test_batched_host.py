"""The one driver behind the five calls that take many clips (batched._BatchedCalls._run_groups), without a GPU: on a model that
was never loaded, with each call's group seam and solo seam replaced by recorders, every clip is sent exactly once, results come
back in input order, a None from the group call sends that group's clips to the solo path, and the decode side sends groups of one
and 'center' clips under two frames solo without trying the group call."""
import dataclasses

import pytest
import torch

HOP = 600
CALLS = ["encode_infer_many", "encode_codes_many", "decode_many", "decode_codes_many", "decode_pcm_many"]


def _tag(t):
    return int(t.reshape(-1)[0])


class _Harness:
    """One of the five calls on stubs.  Clip i is filled with the value i, which is how a stub knows it again; a stub answers
    with that value over the clip's part of the result."""

    def __init__(self, call, refuse=(), padding="same"):
        from wavtokenizer_amd import ARCH_HOP600, WavTokenizer
        self.call, self.refuse, self.encode = call, set(refuse), call.startswith("encode")
        self.m = m = WavTokenizer.from_arch(dataclasses.replace(ARCH_HOP600, padding=padding))
        self.tried, self.grouped, self.solo = [], [], []     # pads of the group calls; clip ids per answered group; per solo call
        m._ensure_engine = lambda: torch.device("cpu")       # (no engine: any real call would fail on the null model handle)
        if call == "encode_infer_many":
            m._run_encode_mixed, m.encode_infer = self.encode_mixed, self.encode_infer
        elif call == "decode_many":
            m._run_decode_mixed, m.decode = self.waves_mixed, lambda f, bandwidth_id=None: self.wave(f[0])
        elif call == "decode_codes_many":
            m._run_decode_codes_mixed, m.decode_codes = self.waves_mixed, lambda c, bandwidth_id=None: self.wave(c)
        elif call == "encode_codes_many":
            m._run_encode_codes_mixed, m._encode_codes_solo = self.codes_mixed, self.codes_solo
        else:
            m._run_decode_pcm_mixed, m._decode_pcm_solo = self.pcm_mixed, self.pcm_solo

    def _group(self, pad, ids):
        """Records a group call; False when this group is refused (the stub then returns None: off route)."""
        self.tried.append(pad)
        if pad not in self.refuse:
            self.grouped.append(ids)
        return pad not in self.refuse

    # encode_infer_many: (features, codes), the codes carry the clip's id
    def encode_mixed(self, wavs, T_pad, dev):
        ids, L = [_tag(w) for w in wavs], self.m.arch.frames(T_pad)
        if not self._group(T_pad, ids):
            return None
        return torch.zeros(len(ids), 512, L), torch.tensor(ids)[None, :, None].expand(1, -1, L)

    def encode_infer(self, wav, bandwidth_id=None):
        L = self.m.arch.frames(wav.shape[1])
        self.solo.append([_tag(wav)])
        return torch.zeros(1, 512, L), torch.full((1, 1, L), _tag(wav))

    # decode_many and decode_codes_many: waveforms whose samples are the clip's id
    def _rows(self, ids, L):
        return torch.tensor(ids, dtype=torch.float32)[:, None].expand(-1, self.m._wave_len(L)).contiguous()

    def waves_mixed(self, clips, L_pad, bw, dev=None):
        ids = [_tag(c) for c in clips]
        return self._rows(ids, L_pad) if self._group(L_pad, ids) else None

    def wave(self, clip):
        self.solo.append([_tag(clip)])
        return self._rows([_tag(clip)], clip.shape[1])

    # encode_codes_many and decode_pcm_many: the clip's id over its span of the flat tensor
    @staticmethod
    def _spans(flat, offs, sizes, ids):
        for off, n, i in zip(offs, sizes, ids):
            flat[off:off + n] = i
        return True

    def codes_mixed(self, specs, T_pad, flat, offs):
        ids = [_tag(sp.clip) for sp in specs]
        return self._spans(flat, offs, [self.m.arch.frames(sp.n_out) for sp in specs], ids) if self._group(T_pad, ids) else None

    def codes_solo(self, specs, flat, offs):
        self.solo.append([_tag(sp.clip) for sp in specs])
        self._spans(flat, offs, [self.m.arch.frames(sp.n_out) for sp in specs], self.solo[-1])

    def pcm_mixed(self, specs, L_pad, bw, flat, offs, fmt, channels_last):
        ids = [_tag(sp.codes) for sp in specs]
        return self._spans(flat, offs, [sp.n_out * sp.channels for sp in specs], ids) if self._group(L_pad, ids) else None

    def pcm_solo(self, specs, bw, flat, offs, fmt, channels_last):
        self.solo.append([_tag(sp.codes) for sp in specs])
        self._spans(flat, offs, [sp.n_out * sp.channels for sp in specs], self.solo[-1])

    def run(self, sizes):
        """The call over clips of these sizes (samples for the encode calls, frames for the decode ones): the clip id found in
        each result, in the order of the results."""
        m = self.m
        if self.encode:
            clips = [torch.full((n,), float(i)) for i, n in enumerate(sizes)]
            out = getattr(m, self.call)(clips)
            codes = [o[1] if self.call == "encode_infer_many" else o for o in out]
            return [int(c[0, 0, 0]) for c in codes], [c.shape[-1] for c in codes]
        if self.call == "decode_many":
            clips = [torch.full((512, n), float(i)) for i, n in enumerate(sizes)]
        else:
            clips = [torch.full((1, n), i, dtype=torch.int64) for i, n in enumerate(sizes)]
        out = getattr(m, self.call)(clips, bandwidth_id=0)
        return [int(o[0, 0]) if o.numel() else None for o in out], [o.shape[-1] for o in out]

    def groups(self, sizes):
        """(groups, solo) as the call's grouping policy gives them: the decode side adds the groups of one and, under 'center'
        padding, the groups that start below two frames."""
        from wavtokenizer_amd.mixed_length import group_clips, group_frames
        if self.encode:
            return group_clips(sizes, HOP)
        low = 1 if self.m.arch.padding == "same" else 2
        every = group_frames(sizes)
        return ([g for g in every if len(g[1]) > 1 and sizes[g[1][0]] >= low],
                [i for _pad, idx in every if len(idx) == 1 or sizes[idx[0]] < low for i in idx])

    def check(self, sizes):
        groups, solo = self.groups(sizes)
        ids, lengths = self.run(sizes)
        per = (lambda n: -(-n // HOP)) if self.encode else self.m._wave_len
        assert lengths == [per(n) for n in sizes]
        # input order, every clip answered by its own result (a 'center' clip of one frame has no samples to look at)
        assert ids == [i if per(n) else None for i, n in enumerate(sizes)]
        assert self.tried == [pad for pad, _idx in groups]                       # every eligible group was tried, no other
        refused = [i for pad, idx in groups if pad in self.refuse for i in idx]
        assert self.grouped == [idx for pad, idx in groups if pad not in self.refuse]
        want_solo = sorted(solo + refused)
        if self.call in ("encode_codes_many", "decode_pcm_many"):                # their solo path takes the sorted remainder at once
            assert self.solo == ([want_solo] if want_solo else [])
        else:
            assert self.solo == [[i] for i in want_solo]
        sent = sorted([i for ids_ in self.grouped for i in ids_] + [i for ids_ in self.solo for i in ids_])
        assert sent == list(range(len(sizes)))                                   # exactly once
        return groups, solo


ENCODE_SIZES = [2000, 2100, 2200, 40000, 41000, 42000, 500, 9000, 1023]         # 500 and 1023: under the mixed-length plans' minimum
DECODE_SIZES = [5, 6, 7, 100, 101, 102, 1, 3000, 31, 33]                        # 3000 forms a group alone


@pytest.mark.parametrize("call", CALLS)
def test_every_clip_is_sent_once_and_results_come_back_in_input_order(call):
    h = _Harness(call)
    groups, solo = h.check(ENCODE_SIZES if h.encode else DECODE_SIZES)
    assert len(groups) >= 2 and solo                                             # (the sizes exercise both paths)
    if not h.encode:
        assert DECODE_SIZES.index(3000) in solo


@pytest.mark.parametrize("call", CALLS)
def test_none_from_the_group_call_sends_its_clips_solo(call):
    probe = _Harness(call)
    sizes = ENCODE_SIZES if probe.encode else DECODE_SIZES
    groups, _solo = probe.groups(sizes)
    h = _Harness(call, refuse=[groups[0][0]])
    h.check(sizes)
    assert h.tried[0] == groups[0][0] and set(groups[0][1]) <= {i for ids in h.solo for i in ids}


@pytest.mark.parametrize("call", [c for c in CALLS if c.startswith("decode")])
def test_decode_side_sends_groups_of_one_and_short_center_clips_solo(call):
    h = _Harness(call)
    h.check([40])                                                                # a group of one never reaches the group call
    assert not h.tried and h.solo == [[0]]
    h = _Harness(call, padding="center")
    h.check([2, 3, 2])                                                           # two frames and more: a group
    assert h.tried == [3] and not h.solo
    h = _Harness(call, padding="center")
    h.check([3, 1, 2])                                                           # a group that starts below two frames (decode raises there)
    assert not h.tried and sorted(i for ids in h.solo for i in ids) == [0, 1, 2]
