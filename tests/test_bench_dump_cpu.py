"""bench.py --dump-outputs on the host side: small outputs are written whole, larger ones cut to a fixed, seeded sample."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_large_outputs_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_OUTPUT_BYTES", 4000)
    arrays = {"x": torch.arange(1000, dtype=torch.float32), "pv": torch.arange(600, dtype=torch.float64).reshape(2, 300),
              "info": torch.tensor([3.0, 20.0, 1.5, 2.5, 0.5, 0.25, 7.0], dtype=torch.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, 0, 1)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert sum(v.nbytes for v in a.values()) <= 4000 and a["x"].dtype == np.float32 and a["pv"].dtype == np.float64
    assert np.array_equal(a["info"], arrays["info"].numpy())           # a small array whole, its fields in place
    assert len(a["x"]) == 493 and len(a["pv"]) == 246                  # the rest of the budget shared evenly by the large ones
    for n in ("x", "pv"):
        v = a[n]
        assert np.all(np.diff(v) > 0) and np.isin(v, arrays[n].numpy()).all()    # positions in increasing order, values kept
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{n}.npy"))
    bench.dump_outputs(str(tmp_path / "r"), arrays, 1, 2)                  # rank 1 of 2: its own names, half the budget
    r = {n: np.load(tmp_path / "r" / f"{n}.rank1.npy") for n in arrays}
    assert sum(v.nbytes for v in r.values()) <= 2000 and np.array_equal(r["info"], arrays["info"].numpy())


def test_dump_outputs_keeps_small_outputs_whole(tmp_path):
    arrays = {"x": torch.arange(10, dtype=torch.float32), "pv": torch.ones((3, 4), dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path), arrays, 0, 1)
    assert sorted(os.listdir(tmp_path)) == ["pv.npy", "x.npy"]
    for n, t in arrays.items():
        assert np.array_equal(np.load(tmp_path / f"{n}.npy"), t.numpy())


def test_dump_outputs_is_refused_with_a_sweep(tmp_path):
    """every count of a sweep would write the same files: the combination is an error"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sweep", "1,2", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--sweep" in out.stderr and os.listdir(tmp_path) == []
