"""The one-product GEMM mode on a host without a GPU: the built library carries the twin's kernels beside the unchanged default
ones, and the header and the Python constants agree on the flag."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel_names():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_table()


def test_library_holds_the_twin_beside_the_default_kernels():
    table = _kernel_names()
    names = " ".join(table)
    assert "gemm16s_kernel<128, 192, 4, 2, 3, 2, 1, 0" in names           # pwconv1's default kernel, name and arguments unchanged
    twins = [n for n in table if "gemm16h_kernel<" in n]
    # eight tile forms for seven (epilogue, output) pairs and two for the head: launch16s_tiled's choices, nothing else
    assert len(twins) == 7 * 8 + 2, len(twins)
    forms = set()
    for n in twins:
        a = [x.strip() for x in re.search(r"gemm16h_kernel<(.*?)>", n).group(1).split(",")]
        assert a[7] == "0", n                                              # no experiment masks
        assert (int(a[5]), int(a[6])) in {(0, 0), (1, 0), (0, 1), (8, 1), (7, 0), (2, 1), (3, 0), (4, 1)}, n     # (Epi, Out16s)
        forms.add((a[0], a[1], a[10], a[11]))
        t = table[n]
        assert not t.get("vgpr_spill_count", 0) and not t.get("private_segment_fixed_size", 0), n
    assert forms == {("256", "64", "1", "0"), ("64", "32", "2", "2"), ("128", "32", "2", "1"), ("128", "32", "1", "0"),
                     ("128", "64", "2", "1"), ("128", "64", "1", "0"), ("128", "128", "1", "0"), ("128", "192", "1", "0")}, forms
    # pwconv1's twin needs fewer registers than the kernel it shadows (no correction accumulators, no lo fragments)
    twin = next(n for n in twins if "gemm16h_kernel<128, 192, 4, 2, 3, 2, 1, 0" in n)
    dflt = next(n for n in table if "gemm16s_kernel<128, 192, 4, 2, 3, 2, 1, 0" in n)
    assert table[twin]["vgpr_count"] < table[dflt]["vgpr_count"]


def test_header_and_python_agree_on_the_flag():
    from wavtokenizer_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "wavtokenizer_amd.h")).read()
    m = re.search(r"WT_PLAN_FLAG_F16_GEMM\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == _capi.WT_PLAN_FLAG_F16_GEMM == 128
    flags = {k: int(v) for k, v in re.findall(r"(WT_PLAN_FLAG_\w+)\s*=\s*(\d+)", hdr)}
    assert len(set(flags.values())) == len(flags)                          # one bit each
    for k, v in flags.items():
        assert getattr(_capi, k) == v, k


def test_python_mode_reaches_only_the_decode_kinds():
    import pytest
    from wavtokenizer_amd import ARCH_HOP600, WavTokenizer, _capi
    m = WavTokenizer.from_arch(ARCH_HOP600)
    F16 = _capi.WT_PLAN_FLAG_F16_GEMM
    assert m._decode_flags(0) == 0
    m.set_gemm_precision("f16")
    assert m._plan_flags & F16 == 0                                        # what the encoder, the head and range_report plan from
    assert m._decode_flags(_capi.WT_PLAN_FLAG_GRAPH) == _capi.WT_PLAN_FLAG_GRAPH | F16
    assert m._decode_flags(_capi.WT_PLAN_FLAG_UNFUSED) == _capi.WT_PLAN_FLAG_UNFUSED
    m._plan_flags |= _capi.WT_PLAN_FLAG_FP32_GEMM
    assert m._decode_flags(m._plan_flags) & F16 == 0
    m.set_gemm_precision("f16x3")
    assert m._decode_flags(0) == 0 and not m._plan_flags & _capi.WT_PLAN_FLAG_FP32_GEMM
    m.set_gemm_precision("f16")
    m.set_gemm_precision("f32")
    assert m._decode_flags(m._plan_flags) == _capi.WT_PLAN_FLAG_FP32_GEMM
    with pytest.raises(ValueError):
        m.set_gemm_precision("bf16")
