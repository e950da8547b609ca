"""CPU: bench.py --dump-outputs' writer -- every array as <name>.npy, whole while they fit the budget, a fixed seeded sample (with its index) beyond it."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _outputs(P=5000, H=64, W=48):
    rng = np.random.default_rng(3)
    out = {"image": rng.standard_normal((3, H, W)).astype(np.float32), "radii": rng.integers(0, 9, P).astype(np.float32)}
    for k, c in (("means3D", 3), ("means2D", 3), ("colors", 3), ("opacities", 1), ("scales", 3), ("rotations", 4)):
        out["grad_" + k] = rng.standard_normal((P, c)).astype(np.float32)
    return out


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_outputs_within_the_budget_are_written_whole(tmp_path):
    arrays = _outputs()
    _bench().dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in arrays)
    for k, a in arrays.items():
        b = np.load(tmp_path / (k + ".npy"))
        assert b.dtype == np.float32 and np.array_equal(a, b), k


def test_outputs_over_the_budget_keep_the_same_seeded_sample(tmp_path):
    arrays = _outputs()
    total = sum(a.nbytes for a in arrays.values())
    budget = total // 4
    bench = _bench()
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, budget=budget)
        assert _size(tmp_path / run) <= budget
    for k, a in arrays.items():
        rows = a.reshape(3, -1).T if k == "image" else a
        idx = np.load(tmp_path / "a" / (k + "_index.npy"))
        assert idx.dtype == np.float64 and len(idx) > 0 and (np.diff(idx) > 0).all()
        got = np.load(tmp_path / "a" / (k + ".npy"))
        assert np.array_equal(got, rows[idx.astype(np.int64)]), k
        assert np.array_equal(got, np.load(tmp_path / "b" / (k + ".npy"))) and np.array_equal(idx, np.load(tmp_path / "b" / (k + "_index.npy"))), k
