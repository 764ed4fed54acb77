"""
bench.py --dump-outputs DIR: what the timed call returned in its last step, as float64 .npy files of at most 64 MB,
keyed by cell id (independent of the order the cells were presented in) -- on a host stand-in for the count matrix.
-m gpu: a plain run (no --full) of a small configuration prints the contract's line, fills nothing that --full
measures, and dumps the same files twice for the same arguments.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("counts_sample", "counts_sample_cells", "cell_totals", "gene_totals", "cell_of_row")


def _load(d, suffix=""):
    return {n: np.load(os.path.join(d, n + suffix + ".npy")) for n in NAMES}


def test_dump_is_keyed_by_cell_and_bounded(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n, G = 3000, 1500
    rng = np.random.default_rng(5)
    x = rng.integers(0, 300, (n, G), dtype=np.int32)
    perm = rng.permutation(n)
    bench.dump_outputs(str(tmp_path / "plan"), torch.from_numpy(x), np.arange(n))
    bench.dump_outputs(str(tmp_path / "perm"), torch.from_numpy(x[perm]), perm, suffix="_rank1")
    a, b = _load(tmp_path / "plan"), _load(tmp_path / "perm", "_rank1")
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in NAMES:
        assert a[name].dtype == np.float64
        if name != "cell_of_row":
            assert np.array_equal(a[name], b[name]), name
    cells = a["counts_sample_cells"].astype(np.int64)
    assert len(cells) == 256 and np.all(np.diff(cells) > 0)
    assert np.array_equal(a["counts_sample"], x[cells])
    assert np.array_equal(a["cell_totals"], x.sum(axis=1))
    assert np.array_equal(a["gene_totals"], x.sum(axis=0))
    assert np.array_equal(b["cell_of_row"], perm)


def test_dump_stays_under_64_mb_on_wide_matrices(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    x = torch.ones((300, 40000), dtype=torch.int32)
    bench.dump_outputs(str(tmp_path), x, np.arange(300))
    d = _load(tmp_path)
    assert d["counts_sample"].shape == ((4 << 20) // 40000, 40000)
    assert sum(v.nbytes for v in d.values()) <= 64 << 20
    for ranks in (2, 8):                                # every rank of N writes its shard's files in a 1/N share
        bench.dump_outputs(str(tmp_path / str(ranks)), x, np.arange(300), suffix="_rank0", ranks=ranks)
        d = _load(tmp_path / str(ranks), "_rank0")
        assert d["counts_sample"].shape == ((4 << 20) // (40000 * ranks), 40000)
        assert sum(v.nbytes for v in d.values()) * ranks <= 64 << 20


def _plain_run(dump_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C2", "--steps", "3", "--warmup", "1",
           "--ramp-ms", "0", "--dump-outputs", str(dump_dir)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-3000:]
    lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, done.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    line = _plain_run(tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["ms_per_step_cold"] is None and line["ms_per_step_unchecked"] is None
    assert "cpu_baseline" not in line and "end_to_end_ms" not in line and "north_star_shape" not in line
    a = _load(tmp_path / "a")
    assert a["counts_sample"].shape == (256, 5000) and a["cell_totals"].shape == (5000,)
    assert a["gene_totals"].sum() > 0
    _plain_run(tmp_path / "b")
    b = _load(tmp_path / "b")
    for name in NAMES:
        assert np.array_equal(a[name], b[name]), name
