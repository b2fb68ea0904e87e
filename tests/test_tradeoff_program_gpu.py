"""-m gpu: DAzimSurfTomo_amd's third argument, tradeoff = K (tradeoff.dat from dazim_model_tradeoff on the last outer iteration's matrix
and right-hand side), on test1's inputs as tests/test_model_uncertainty_program_gpu.py runs them (17 x 17 x 4, n = 675 in iso-mode T
and 2 025 in F), two iterations, both iso-modes, K = 5."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_phase_map_program_gpu import INV, build, inputs, run

pytestmark = pytest.mark.gpu

K = 5
TRADE = "tradeoff.dat"
LOG = "para.in_inv.log"
WEIGHT_VS, WEIGHT_GCS, DAMP = 2.0, 2.0, 0.0     # para.in of tests/test_phase_map_program_gpu.py
FACTORS = 10.0 ** (-1.0 + 2.0 * np.arange(K) / (K - 1))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """per iso-mode: (directory of a run without the arguments, directory of a run with uncertainty 0 and tradeoff K, that run's stdout)"""
    build()
    out = {}
    for iso in ("T", "F"):
        plain, trade = tmp_path_factory.mktemp("plain" + iso), tmp_path_factory.mktemp("trade" + iso)
        run(INV, plain, inputs(maxiter=2, iso=iso))
        out[iso] = (plain, trade, run(INV, trade, inputs(maxiter=2, iso=iso), "0", str(K)))
    return out


def columns(iso):
    """tradeoff.dat's columns by name: sweep, factor, weights per block, damp, chi2, reg2 per block, xnorm2, dof per block, gcv, logev"""
    nblk = 1 if iso == "T" else 3
    names = ["sweep", "factor"] + [f"w{b}" for b in range(nblk)] + ["damp", "chi2"] + [f"reg2_{b}" for b in range(nblk)] + ["xnorm2"] + \
        [f"dof{b}" for b in range(nblk)] + ["gcv", "logev"]
    return nblk, {n: i for i, n in enumerate(names)}


@pytest.mark.parametrize("iso", ["T", "F"])
def test_tradeoff_file(runs, iso):
    """K lines in iso-mode T and 2K in F, all finite; the factors; factor 1 has para.in's weights; along a sweep the regularisation
    norm of the swept blocks does not increase and what the sweep holds fixed (chi2, the damping being 0, plus in sweep 2 the Vs block's
    term) does not decrease; the resolved parameters lie in (0, n) and fall as the weights rise; three log lines per sweep, each naming
    a point of the sweep.
    Measured on an MI355X (factors 0.1 .. 10): iso-mode T sum of dof 49.7, 29.1, 11.4, 2.5, 0.3 of n 675, corner and evidence at factor
    1, GCV at 0.32; iso-mode F sweep 1 sum of dof 65.0, 43.9, 20.9, 5.7, 0.8 of n 2 025, sweep 2 61.5, 41.2, 20.9, 11.5, 9.7; in both
    sweeps the corner at factor 3.2, GCV at 0.32, the evidence at 1 (log evidence -121.8 against -147.7 and -131.6 beside it in sweep 1, -143.1 and -122.4 in sweep 2)."""
    plain, trade, stdout = runs[iso]
    nblk, col = columns(iso)
    nsweep = 1 if iso == "T" else 2
    assert not (plain / TRADE).exists()
    a = np.loadtxt(trade / TRADE, ndmin=2)
    assert a.shape == (nsweep * K, len(col)) and len((trade / TRADE).read_text().splitlines()) == nsweep * K
    assert np.isfinite(a).all()
    assert np.array_equal(a[:, col["sweep"]], np.repeat(np.arange(1, nsweep + 1), K))
    n = nblk * 15 * 15 * 3
    for s in range(nsweep):
        b = a[s * K:(s + 1) * K]
        assert np.allclose(b[:, col["factor"]], FACTORS, rtol=1e-6)
        one = b[K // 2]
        assert one[col["factor"]] == 1.0 and one[col["w0"]] == WEIGHT_VS and (b[:, col["damp"]] == DAMP).all()
        if nblk == 3:
            assert one[col["w1"]] == WEIGHT_GCS and one[col["w2"]] == WEIGHT_GCS
            assert np.allclose(b[:, col["w1"]], WEIGHT_GCS * FACTORS, rtol=1e-6) and np.array_equal(b[:, col["w1"]], b[:, col["w2"]])
        assert np.allclose(b[:, col["w0"]], WEIGHT_VS * (FACTORS if s == 0 else 1.0), rtol=1e-6)
        swept = [f"reg2_{k}" for k in range(nblk)][(0 if s == 0 else 1):]
        reg2 = b[:, [col[k] for k in swept]].sum(axis=1)
        chi2 = b[:, col["chi2"]]
        held = chi2 + (0.0 if s == 0 else b[:, col["reg2_0"]])     # (the rows are stored at para.in's weights: scale 1 on the Vs block)
        assert (np.diff(reg2) <= 1e-6 * reg2.max()).all() and (np.diff(held) >= -1e-6 * held.max()).all()
        dof = b[:, [col[f"dof{k}"] for k in range(nblk)]].sum(axis=1)
        assert (dof > 0).all() and (dof < n).all() and (np.diff(dof) < 0).all() and (b[:, col["gcv"]] > 0).all()
        print(f"\n[measured] iso-mode {iso} sweep {s + 1}: sum of dof per factor " + " ".join(f"{v:.1f}" for v in dof) + f" of n {n}; chi2 " +
              " ".join(f"{v:.4e}" for v in chi2) + "; logev " + " ".join(f"{v:.5e}" for v in b[:, col["logev"]]))
    if nsweep == 2:                                          # the two sweeps meet at factor 1: the same point
        assert np.array_equal(a[K // 2, 2:], a[K + K // 2, 2:])
    for text in ((trade / LOG).read_text(), stdout):
        lines = [ln for ln in text.splitlines() if ln.startswith(" tradeoff sweep")]
        assert len(lines) == 3 * nsweep, lines
        for s in range(nsweep):
            for ln, what in zip(lines[3 * s:3 * s + 3], ("L-curve corner", "GCV minimum", "evidence maximum")):
                assert ln.startswith(f" tradeoff sweep {s + 1} (") and what + " at point" in ln, ln
                point = int(ln.split("at point")[1].split(",")[0])
                assert 1 <= point <= K and (what != "L-curve corner" or 1 < point < K)
        print("\n[measured] " + "\n[measured] ".join(lines))
    assert "tradeoff" not in (plain / LOG).read_text()


@pytest.mark.parametrize("iso", ["T", "F"])
def test_other_files_are_byte_identical(runs, iso):
    """the model the program inverts with is not changed: every other file has the bytes of the run without the arguments"""
    plain, trade, _ = runs[iso]
    names = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in trade.iterdir()) == sorted(names + [TRADE])
    strip = lambda text: [ln for ln in text.splitlines() if "time cost" not in ln and not ln.startswith(" tradeoff")]
    for n in names:
        if n.endswith(".log"):
            assert strip((plain / n).read_text()) == strip((trade / n).read_text()), n
        else:
            assert (plain / n).read_bytes() == (trade / n).read_bytes(), n


def test_tradeoff_zero_is_the_plain_run(runs, tmp_path):
    plain = runs["T"][0]
    stdout = run(INV, tmp_path, inputs(maxiter=2, iso="T"), "0", "0")
    assert not (tmp_path / TRADE).exists() and "tradeoff" not in stdout and "tradeoff" not in (tmp_path / LOG).read_text()
    assert (plain / "DSurfTomo.inv").read_bytes() == (tmp_path / "DSurfTomo.inv").read_bytes()


def test_fewer_than_three_points_are_refused(tmp_path):
    build()
    for name, text in inputs(maxiter=1, iso="T").items():
        (tmp_path / name).write_text(text)
    out = subprocess.run([INV, "para.in", "0", "2"], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert out.returncode != 0 and any(ln.startswith(" ERROR: tradeoff is 0 or the number of sweep points") for ln in out.stdout.splitlines())
    assert not (tmp_path / "IterVel.out").exists() and not (tmp_path / TRADE).exists()


def test_more_than_one_rank_is_refused(tmp_path):
    """the matrix of a multi-rank run is row-sharded: with the argument the program stops before any rank is started"""
    build()
    for name, text in inputs(maxiter=1, iso="T").items():
        (tmp_path / name).write_text(text)
    out = subprocess.run([INV, "para.in", "0", str(K)], cwd=tmp_path, timeout=300, capture_output=True, text=True,
                         env=dict(os.environ, DAZIM_NGPU="2"))
    assert out.returncode != 0, out.stdout[-2000:]
    assert any(ln.startswith(" ERROR: tradeoff > 0 needs the whole matrix on one GPU") for ln in out.stdout.splitlines()), out.stdout[-2000:]
    assert not (tmp_path / "IterVel.out").exists() and not (tmp_path / TRADE).exists()
