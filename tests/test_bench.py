"""bench.py end to end on the GPU: a plain run carries the headline and nothing that needs a run of its own; --full adds the
one-stream block and its roofline launch timing.  Short child processes (2 timed steps), one per mode."""
import json
import os
import subprocess
import sys

import pytest

from tests.util import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = (r.stdout or "")[-2000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, tail
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_only():
    d = _bench()
    for k in HEADLINE:
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "audio-s/s" and d["higher_is_better"] is True and d["dtype"] == "f32 (split-f16 x3 products)"
    assert d["config"]["lanes"] == 2
    for k in ("roofline", "cpu_baseline", "speedup_vs_cpu", "other_configs"):
        assert k not in d, k
    assert "one_lane" not in d["config"]


def test_bench_full_adds_the_one_lane_block_and_the_roofline():
    d = _bench("--full", "--no-cpu-baseline", "--no-other-configs")
    for k in HEADLINE:
        assert k in d, k
    assert d["config"]["lanes"] == 2 and d["config"]["one_lane"]["ms_per_step"] > 0
    assert d["roofline"]["launches_timed"] > 0 and d["roofline"]["achieved"] > 0
    assert "cpu_baseline" not in d and "other_configs" not in d
