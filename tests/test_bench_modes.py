"""bench.py's two kinds of run.  A plain run does what its line's headline needs and nothing more: no text passes, no CPU baselines,
no extra records, and its index is built in a directory of its own that is gone when it exits.  --full adds those measurements next to
the same timed steps."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.delenv("DSM_BENCH_DIR", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.workdir is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True


def _line(extra, env):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--reads", "200000", "--genome", "1000000"] + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_adds_the_rest(tmp_path):
    env = dict(os.environ, TMPDIR=str(tmp_path))
    env.pop("DSM_BENCH_DIR", None)
    plain = _line([], env)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("dsm_bench.")]   # the run's own index directory went with it
    assert "cpu_baseline" not in plain and "extra_records" not in plain
    assert plain["detail"]["text_pass_ms"] is None and plain["detail"]["format_ms_per_step"] is None
    full = _line(["--full", "--cpu-seconds", "1"], env)
    assert full["cpu_baseline"]["value"] > 0
    assert full["detail"]["text_pass_ms"] > 0 and full["detail"]["format_ms_per_step"] > 0
    assert full["detail"]["text_pass_bytes"] == full["detail"]["format_text_bytes_per_step"] > 0
    assert "extra_records" not in full   # (they need a sample of at least 10^6 reads)
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup"):
        assert plain[k] == full[k], k
    for k in ("rank0_nodes_per_step", "tuples_per_step", "union_nodes_per_step", "candidates_per_step", "rank_ops_per_node"):
        assert plain["detail"][k] == full["detail"][k] > 0, k
