"""RCCL for real on the one GPU a test box has ("RCCL all-reduce of gradients over xGMI in training",
the fit of given_others_gt_mean_var_seq2seq.py:494-506).  The worker runs as a CHILD process - started before it touches the
GPU - with backend "nccl" (= RCCL on ROCm) at world size 1 and FOV_FORCE_DIST=1, which sends the trainers through their
data-parallel branch: async tail all-reduce under the encoder BPTT, poison slot + head all-reduce, work.wait(), guarded
optimizer; parallel.broadcast_index on the nccl backend."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forced_data_parallel_over_rccl_equals_plain_path():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("FOV_FORCE_DIST", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dist_nccl_worker.py")], env=env, capture_output=True,
                       text=True, timeout=900)
    print(r.stdout[-4000:])
    print(r.stderr[-4000:])
    assert r.returncode == 0, "worker failed"
    assert "DIST_NCCL_WORKER OK" in r.stdout
    for name in ("mixing_f32", "mixing_bf16", "seq2seq"):
        assert "%s: forced-DP over RCCL == plain path: True" % name in r.stdout


def _bench_two_ranks(extra_env, timeout):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", FOV_DP_PROBE_BATCH="32", **extra_env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "FOV_FORCE_DIST"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--batch", "64",
                           "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full"], env=env, capture_output=True, text=True, timeout=timeout)


def _json_line(stdout):
    import json
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_rehearsal_carries_the_data_parallel_probe():
    """The N > 1 form of bench.py --full end to end on the one GPU of the box (two ranks over gloo, small batches so that both ranks'
    persistent grids are co-resident): rank 0's ONE line has n_gpus 2, the whole-job value, and under `extra` the data-parallel
    training probe's step and all-reduce times for fp32 and for bf16."""
    r = _bench_two_ranks({}, 900)
    print(r.stderr[-3000:])
    assert r.returncode == 0
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 128 and d["value"] > 0
    x = d["extra"]
    assert "error" not in x, x
    for leg in (x, x["bf16"]):
        assert leg["dp_step_ms"] > 0 and leg["allreduce_ms"] > 0 and leg["allreduce_payload_bytes"] == 4 * (4 + 1678036 + 1), leg
        assert 0 < leg["final_loss"] < 1.0


def test_bench_probe_watchdog_fails_the_run_but_prints_the_headline():
    """A collective of the probe that never completes (rank 1 never arrives: test hook): after FOV_DP_PROBE_LIMIT_S every rank
    leaves with exit code 3 - the launcher reports failure - and rank 0 has printed the headline line with the error under
    `extra` (round-4 verdict: the watchdog used to exit 0)."""
    r = _bench_two_ranks({"FOV_DP_PROBE_TEST_HANG": "1", "FOV_DP_PROBE_LIMIT_S": "20"}, 600)
    print(r.stderr[-3000:])
    assert r.returncode != 0
    d = _json_line(r.stdout)
    # (rank 0's own watchdog fires - "did not finish" - or rank 1's fires first and rank 0's collective raises: either way an error)
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["extra"].get("error")
