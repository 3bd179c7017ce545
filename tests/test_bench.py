"""bench.py's two kinds of run: a plain run prints the headline line and nothing it does not need; `--full` adds the records
measured after the timed steps (collective, roofline, cpu_baseline, targets ...)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _parse(monkeypatch, *argv):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_is_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1")
    assert not a.full and (a.steps, a.warmup) == (3, 1)
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--no-targets")
    assert a.full and a.no_cpu_baseline and a.no_targets and not a.no_roofline


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", *argv],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    for k in HEADLINE:
        assert k in rec, k
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["steps"] == 3 and rec["warmup"] == 2
    assert rec["higher_is_better"] is True and rec["dtype"] == "f32" and rec["unit"] == "patches/s"
    return rec


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone():
    rec = _bench()
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["collective"] is None
    for k in ("targets", "c2", "train_loop", "c5", "z32ex"):
        assert k not in rec, k
    assert set(rec["final_losses"]) == {"recon", "commitment", "total", "perplexity"}


@pytest.mark.gpu
def test_full_run_adds_the_records_after_the_timed_steps():
    rec = _bench("--full", "--no-cpu-baseline", "--no-targets")
    assert rec["roofline"]["bound"] == "hbm" and rec["roofline"]["achieved"] > 0
    assert rec["collective"]["world"] == 1 and rec["collective"]["replicas_bit_equal"] is True
    assert rec["cpu_baseline"] is None and "targets" not in rec
