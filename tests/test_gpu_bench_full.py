"""bench.py --full: the headline line plus everything else the default mode measures and checks after its timed steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_run_adds_the_breakdown_parity_large_batch_and_cpu_baseline():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full",
                        "--cpu-budget", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["value"] > 0 and res["ms_per_step"] > 0
    k = res["kernels"]
    assert k["encoder_ms"] > 0 and k["decoder_ms"] > 0
    p = res["parity"]
    assert p["sequences_checked"] == 64 and p["max_abs_err_vs_oracle"] < 1e-4 and p["decoder_only_call_equals_fused_call"]
    assert p["max_abs_err_vs_torch_cpu"] < 1e-4
    lb = res["large_batch"]
    assert lb["batch"] == 4096 and lb["ms_per_call"] > 0 and lb["max_abs_err_vs_oracle"] < 1e-4
    cpu = res["cpu_baseline"]
    assert cpu["value"] > 0 and cpu["legs"]
    assert res["speedup_vs_cpu_baseline"] == pytest.approx(res["value"] / cpu["value"])
