"""bench.py's command line without a GPU: what a plain run leaves out (everything behind --full), --steps, and the
--dump-outputs writer (float32 .npy files, a seeded sample of the same fraction of every array above the size budget)."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return load_bench().parse_args()


def test_plain_run_leaves_the_extra_measurements_to_full(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    assert a.no_verify and a.no_extras and a.no_cpu_baseline and a.per_matrix_reps == 0
    f = parse(monkeypatch, "--steps", "7", "--full", "--dump-outputs", "out")
    assert f.full and f.dump_outputs == "out"
    assert not f.no_verify and not f.no_extras and not f.no_cpu_baseline and f.per_matrix_reps == 10
    assert parse(monkeypatch, "--full", "--no-cpu-baseline").no_cpu_baseline
    assert parse(monkeypatch, "--full", "--per-matrix-reps", "3", "--details", "d.json").per_matrix_reps == 3
    assert parse(monkeypatch, "--per-matrix-reps", "0").per_matrix_reps == 0


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--steps", "0")


@pytest.mark.parametrize("argv", [["--per-matrix-reps", "5"], ["--details", "d.json"], ["--per-matrix-reps", "0", "--details", "d.json"]])
def test_per_matrix_table_needs_full(monkeypatch, argv):
    """What only --full measures, asked for without it: an error, never an empty table."""
    with pytest.raises(SystemExit):
        parse(monkeypatch, *argv)


def test_dump_outputs_writes_float32_arrays(tmp_path):
    bench = load_bench()
    y = {"y_a": np.arange(10, dtype=np.float64) / 3, "y_b/c": np.ones(4, np.float32)}
    assert bench.dump_outputs(y, tmp_path / "d") == {"y_a": 10, "y_b_c": 4}
    a = np.load(tmp_path / "d" / "y_a.npy")
    assert a.dtype == np.float32 and np.array_equal(a, y["y_a"].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "d" / "y_b_c.npy"), y["y_b/c"])


def test_dump_outputs_samples_alike_above_the_budget(tmp_path):
    bench = load_bench()
    y = {"y_big": np.arange(3000, dtype=np.float32), "y_small": np.arange(1000, dtype=np.float32)}
    n1 = bench.dump_outputs(y, tmp_path / "1", budget_bytes=8000)
    n2 = bench.dump_outputs(y, tmp_path / "2", budget_bytes=8000)
    assert n1 == n2 == {"y_big": 1500, "y_small": 500}
    assert sum(4 * n for n in n1.values()) <= 8000
    for name in n1:
        s1, s2 = np.load(tmp_path / "1" / f"{name}.npy"), np.load(tmp_path / "2" / f"{name}.npy")
        assert np.array_equal(s1, s2) and np.all(np.diff(s1) > 0) and np.isin(s1, y[name]).all()
