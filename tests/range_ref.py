"""Shared by tests/test_range_sites.py: the decoder's range sites in plan order, the site masks the tests force, the dead-channel
weight edits that push one S32 tensor beyond the f16 range, and the float64 references.  Everything here runs on the CPU and
nothing comes from a kernel output."""
import numpy as np
import torch

from tests.util import rel_l2, synth_state_dict

BW = torch.tensor([0])
BAR_ABS = 2e-5          # test_precision_against_float64: the shipped path's rel-L2 from the float64 oracle
BAR_RATIO = 4.0         # ... and its multiple of the CPU fp32 oracle's own distance from float64 on the same input
OVER = 1e5              # beyond 65504, the largest finite f16


# ------------------------------------------------------------------------------------------------------- sites
def decoder_sites(arch):
    """[(site, label)] of build_decode, in plan order."""
    from wavtokenizer_amd import _capi as c
    sites = [(c.WT_SITE_BB_EMBED, "embed"), (c.WT_SITE_RES0, "res0"), (c.WT_SITE_RES1, "res1"), (c.WT_SITE_ATTN, "attn"),
             (c.WT_SITE_RES2, "res2"), (c.WT_SITE_RES3, "res3")]
    sites += [(c.WT_SITE_CNX0 + i, "cnx%d" % i) for i in range(arch.num_layers)]
    sites.append((c.WT_SITE_HEAD, "head"))
    assert len(sites) == 7 + arch.num_layers and [s for s, _ in sites] == sorted(s for s, _ in sites)
    return sites


def site_masks(arch):
    """[(label, mask)]: every site alone, every adjacent pair in plan order, all decoder sites."""
    sites = decoder_sites(arch)
    out = [(n, 1 << s) for s, n in sites]
    out += [(a + "+" + b, (1 << sa) | (1 << sb)) for (sa, a), (sb, b) in zip(sites, sites[1:])]
    out.append(("all", sum(1 << s for s, _ in sites)))
    return out


def all_decoder_sites(arch):
    return site_masks(arch)[-1][1]


# ---------------------------------------------------------------------------------------------------- references
def features(B, L):
    """randn * 0.5, the scale of the existing range test; (2, 50) is that test's tensor."""
    seed = 9 if (B, L) == (2, 50) else 1000 * B + L
    return torch.randn(B, 512, L, generator=torch.Generator().manual_seed(seed)) * 0.5


def oracles(arch_name, sd):
    """(fp32 oracle, float64 oracle on the same weights cast up)."""
    from oracle.cpu_ref import OracleWavTokenizer
    from wavtokenizer_amd import NAMED_ARCHS
    arch = NAMED_ARCHS[arch_name]
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    return OracleWavTokenizer(arch, t), OracleWavTokenizer(arch, {k: (v.double() if v.is_floating_point() else v) for k, v in t.items()})


def decode_reference(arch_name, sd, feats):
    """{"w64": the float64 oracle's waveform on the fp32 features cast up, "e_cpu": the fp32 oracle's rel-L2 from it,
    "taps": the fp32 oracle's stage taps}."""
    o32, o64 = oracles(arch_name, sd)
    taps = {}
    with torch.inference_mode():
        w64 = o64.decode(feats.double(), BW)
        w32 = o32.decode(feats, BW, taps)
    assert w64.dtype == torch.float64 and w32.dtype == torch.float32 and bool(torch.isfinite(w64).all())
    return {"w64": w64.numpy(), "e_cpu": rel_l2(w32.numpy(), w64.numpy()), "taps": taps}


_REFS = {}


def reference(arch_name, B, L):
    """decode_reference on the synthetic weights and features(B, L): computed once, shared, never modified."""
    if (arch_name, B, L) not in _REFS:
        _REFS[(arch_name, B, L)] = decode_reference(arch_name, synth_state_dict(arch_name), features(B, L))
    return _REFS[(arch_name, B, L)]


def float64_bars(got, ref, what):
    """The two bars test_precision_against_float64 sets for the shipped path; returns the rel-L2."""
    e = rel_l2(np.asarray(got), ref["w64"])
    print(f"{what}: rel-L2 from float64 {e:.3e} ({e / ref['e_cpu']:.2f} x the CPU fp32 oracle's {ref['e_cpu']:.3e})")
    assert e < BAR_ABS, (what, e)
    assert e < BAR_RATIO * ref["e_cpu"], (what, e, ref["e_cpu"])
    return e


# --------------------------------------------------------------------------------------------- dead-channel edits
# One channel of the affine that feeds a site's first S32 producer gets +1e5, and the column that reads that channel is zeroed
# in every weight that reads the tensor: the S32 tensor holds a value beyond 65504 (so the site must report), and in exact
# arithmetic the output is that of the model without the channel, as well-conditioned as the unedited one.
CHANNEL = 5


def _bump(sd, key, idx):
    v = sd[key].copy()
    v[idx] += np.float32(OVER)
    sd[key] = v


def _zero(sd, key, idx):
    v = sd[key].copy()
    v[idx] = 0.0
    sd[key] = v


def dead_channel_edits(arch):
    """[label] of the edits, in plan order of their sites."""
    return ["embed", "res0", "attn", "res3", "cnx0", "cnx%d" % (arch.num_layers - 1), "head"]


def dead_channel(arch_name, label, feats):
    """(site, edited state dict, edited features) of one edit on the synthetic weights; the inputs are not modified."""
    from wavtokenizer_amd import NAMED_ARCHS, _capi as c
    arch = NAMED_ARCHS[arch_name]
    sd = dict(synth_state_dict(arch_name))
    ch = CHANNEL
    if label == "embed":                         # the transpose writes the features themselves in S32
        feats = feats.clone()
        feats[:, ch, :] = OVER
        _zero(sd, "backbone.embed.weight", (slice(None), ch))
        return c.WT_SITE_BB_EMBED, sd, feats
    if label == "res0":                          # swish(GroupNorm 1) of the block: bb.h1 as conv1 reads it
        _bump(sd, "backbone.pos_net.0.norm1.bias", ch)
        _zero(sd, "backbone.pos_net.0.conv1.weight", (slice(None), ch))
        return c.WT_SITE_RES0, sd, feats
    if label == "res3":                          # swish(GroupNorm 2): the second use of bb.h1 in a block
        _bump(sd, "backbone.pos_net.4.norm2.bias", ch)
        _zero(sd, "backbone.pos_net.4.conv2.weight", (slice(None), ch))
        return c.WT_SITE_RES3, sd, feats
    if label == "attn":                          # the normalised input of q, k and v
        _bump(sd, "backbone.pos_net.2.norm.bias", ch)
        for w in ("q", "k", "v"):
            _zero(sd, "backbone.pos_net.2.%s.weight" % w, (slice(None), ch))
        return c.WT_SITE_ATTN, sd, feats
    if label.startswith("cnx"):                  # the GELU output between pwconv1 and pwconv2
        i = int(label[3:])
        _bump(sd, "backbone.convnext.%d.pwconv1.bias" % i, ch)
        _zero(sd, "backbone.convnext.%d.pwconv2.weight" % i, (slice(None), ch))
        return c.WT_SITE_CNX0 + i, sd, feats
    if label == "head":                          # the final LayerNorm's output, the head's operand
        _bump(sd, "backbone.final_layer_norm.bias", ch)
        _zero(sd, "head.out.weight", (slice(None), ch))
        return c.WT_SITE_HEAD, sd, feats
    raise KeyError(label)


_EDITED = {}


def edited(arch_name, label):
    """(site, edited state dict, edited features (2, 50), decode_reference on them): computed once, shared, never modified."""
    if (arch_name, label) not in _EDITED:
        site, sd, feats = dead_channel(arch_name, label, features(2, 50))
        _EDITED[(arch_name, label)] = (site, sd, feats, decode_reference(arch_name, sd, feats))
    return _EDITED[(arch_name, label)]
