"""CPU: tests/host/packed_section_check.cpp, compiled host-only next to the library (csrc/Makefile) and run here.  It drives
the packed image's model section (wavtokenizer_amd/csrc/packed.cpp: the one walk over the model, the archive, the validator,
the lister) on synthetic models:
round trip, truncation, every listed array with its allocation one word short, every architecture-fixed field off by one, and
the crafted records and lazy entries an image could hold.  No GPU, no image, no hash.

`python -m tests.test_packed_section_host FILE` writes the program's input alone (the Makefile's sanitizer target reads it)."""
import ctypes
import dataclasses
import os
import re
import subprocess
import sys

from tests import weights_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wavtokenizer_amd", "csrc")
CNX_ARRAYS = 9               # dw_w, dw_b, ada_s, ada_h, W1, b1, W2, b2, gamma


def _cases():
    """[(name, arch, with SEANetDecoder)]: the four models of tests/test_model_weights.py, and the reduced one of
    tests/test_weight_checks.py, whose state dict (shared with that module) is small enough to count weights_ref's arrays here."""
    from wavtokenizer_amd import NAMED_ARCHS
    from tests.test_weight_checks import _case
    h6, h3 = NAMED_ARCHS["hop600"], NAMED_ARCHS["hop320"]
    return [("hop600", h6, False), ("hop320", h3, False), ("hop600+seanet", h6, True),
            ("hop600x3", dataclasses.replace(h6, num_quantizers=3), False), ("reduced", _case()[0], True)]


def write_archs(path):
    """(wt_arch, int32 has_seadec) records, as _Engine.load fills a wt_arch."""
    from wavtokenizer_amd._capi import WtArch
    with open(path, "wb") as f:
        for _name, arch, seadec in _cases():
            wa = WtArch()
            wa.n_ratios = len(arch.ratios)
            for i, r in enumerate(arch.ratios):
                wa.ratios[i] = int(r)
            wa.vq_bins, wa.num_quantizers, wa.input_channels = arch.vq_bins, arch.num_quantizers, arch.input_channels
            wa.dim, wa.intermediate_dim, wa.num_layers = arch.dim, arch.intermediate_dim, arch.num_layers
            wa.adanorm_num_embeddings = arch.adanorm_num_embeddings
            wa.n_fft, wa.hop_length = arch.n_fft, arch.hop_length
            wa.padding_same = 1 if arch.padding == "same" else 0
            f.write(bytes(wa) + bytes(ctypes.c_int32(1 if seadec else 0)))


def test_packed_section_check_program(tmp_path):
    """Exit status 0 (every refusal happened, with the message that names the array or field), and the counts: the program
    tried every array its lister names; for the reduced model that is weights_ref.expected's set plus one S32 copy per array a
    copy can stand for; the full SEANetDecoder model differs from hop320's reduced one by its ten further ConvNeXt blocks only."""
    from tests.test_weight_checks import _case
    archs = str(tmp_path / "archs.bin")
    subprocess.run(["make", "-C", CSRC, "build/packed_section_check"], check=True, stdout=subprocess.DEVNULL)      # build() has made it
    exe = os.path.join(CSRC, "build", "packed_section_check")
    write_archs(archs)
    run = subprocess.run([exe, archs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "all checks held" in run.stdout, run.stdout[-2000:]
    rows = re.findall(r"arch (\d+): arrays (\d+) \(fp32/LSTM (\d+), S32 copies (\d+)\) lister (\d+), pods (\d+), mutations (\d+)", run.stdout)
    cases = _cases()
    assert [int(r[0]) for r in rows] == list(range(len(cases)))
    got = {}
    for (name, _arch, _sea), r in zip(cases, rows):
        tried, plain, copies, lister, pods, mutations = (int(x) for x in r[1:])
        assert tried == lister == plain + copies and pods > 100 and mutations >= 2 * pods + 20, (name, r)
        got[name] = plain
    arch, sd = _case()
    assert got["reduced"] == len(W.expected(arch, sd))
    assert got["hop600+seanet"] == got["reduced"] + CNX_ARRAYS * (cases[2][1].num_layers - arch.num_layers)
    assert got["hop600"] == got["hop320"] == got["hop600x3"] < got["hop600+seanet"]


if __name__ == "__main__":
    write_archs(sys.argv[1])
