"""A plain bench.py run on one GPU (no --full): the headline fields with exactly --steps timed steps and none of the --full
figures; --dump-outputs holds the y of the last timed step, checked against a host fp64 product of the same inputs (the
matrices of hispmv_amd.matrices.benchmark_set, x and b from bench.py's own step_vectors)."""
import importlib.util
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from util import bwd_err

pytestmark = pytest.mark.gpu


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def host_csr(m):
    """(rp, ci, va, rows, cols) of a benchmark matrix: the stand-in's arrays, or a real .mtx file through the reader the
    benchmark's handle is created with (flavour 1)."""
    if "path" in m:
        from hispmv_amd.prep import prep_from_mtx
        pr = prep_from_mtx(m["path"], 1)
        return pr.row_ptr, pr.col_idx, pr.values, pr.rows, pr.cols
    return m["rp"], m["ci"], m["va"], m["rows"], m["cols"]


def test_plain_line_and_dumped_outputs(tmp_path):
    import scipy.sparse as sp
    from hispmv_amd import matrices as M
    bench = load_bench()
    names = ["crankseg_2", "ford2"]
    out = tmp_path / "dump"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--preheat", "0.01",
           "--matrices", ",".join(names), "--dump-outputs", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1200:])
    line = [q for q in p.stdout.splitlines() if q.startswith("{") and '"metric"' in q]
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "GFLOP/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"].startswith("SpMV GFLOP/s")
    assert d["cpu_baseline"] is None and d["rank_breakdown"] is None and d["y_checked"] is None and "strong_scaling" not in d
    assert sorted(q.name for q in out.iterdir()) == sorted(f"y_{n}.npy" for n in names)
    for idx, m in enumerate(M.benchmark_set(names)):                 # handles are numbered in load order
        rp, ci, va, rows, cols = host_csr(m)
        y = np.load(out / f"y_{m['name']}.npy")
        assert y.dtype == np.float32 and y.shape == (rows,)
        x, b = (v.numpy().astype(np.float64) for v in bench.step_vectors(idx, rows, cols))
        A = sp.csr_matrix((np.asarray(va, np.float64), ci, rp), shape=(rows, cols))
        y64 = bench.ALPHA * (A @ x) + bench.BETA * b
        A.data = np.abs(A.data)
        assert bwd_err(y, y64, abs(bench.ALPHA) * (A @ np.abs(x)) + abs(bench.BETA) * np.abs(b)) < 1e-5
