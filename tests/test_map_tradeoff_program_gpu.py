"""-m gpu: SurfPhaseMaps_amd para.in weight_c weight_a uncertainty tradeoff on test1's inputs (tests/test_phase_map_program_gpu.py):
map_tradeoff.dat and the log's pick lines of the trade-off sweep (dazim_map_tradeoff), two iterations, weights
2.0, K = 5, iso-mode T and F; every other file as without the argument."""
import os

import numpy as np
import pytest

from tests import test_phase_map_program_gpu as prog

pytestmark = pytest.mark.gpu

K = 5
KMAX = prog.KMAX
SLACK = 1e-9


@pytest.mark.parametrize("iso", ["T", "F"])
def test_map_tradeoff_dat_and_nothing_else_changes(tmp_path, iso):
    """nsweep (KMAX + 1) K lines of 9 + 3 nblk columns, every value finite; in sweep 1 (one factor on all blocks, test1 has no damping:
    a one-parameter Tikhonov family), per period and in the totals, chi2 does not decrease with the factor and sum reg2 and sum dof do
    not increase (slack 1e-9 relative); the total lines' chi2 and logev are the sums of the period lines, to the printed digits; the
    log carries three pick lines per sweep and period and for the totals; every other file is byte-identical to a run without the
    argument (lines with a wall time aside), which writes no map_tradeoff.dat.  The picks per period are printed, not asserted."""
    prog.build()
    files = prog.inputs(maxiter=2, iso=iso)
    prog.run(prog.MAPS, tmp_path / "plain", files, "2.0", "2.0")
    out = prog.run(prog.MAPS, tmp_path / "sweep", files, "2.0", "2.0", "0", str(K))
    nblk, nsw = (1, 1) if iso == "T" else (3, 2)
    tab = np.loadtxt(tmp_path / "sweep" / "map_tradeoff.dat", ndmin=2)
    assert tab.shape == (nsw * (KMAX + 1) * K, 9 + 3 * nblk) and np.isfinite(tab).all(), tab.shape
    # (c_w: the last block's weight, swept in both sweeps)
    c_fac, c_w, c_mp, c_chi2, c_reg, c_dof, c_lev = 2, 2 + nblk, 4 + nblk, 5 + nblk, 6 + nblk, 7 + 2 * nblk, 8 + 3 * nblk
    factors = 10.0 ** (-1 + 2 * np.arange(K) / (K - 1))
    for s in range(1, nsw + 1):
        rows = tab[tab[:, 0] == s].reshape(KMAX + 1, K, -1)                    # periods 1 .. KMAX, then the totals
        assert (rows[:, :, 1] == np.r_[1:KMAX + 1, 0][:, None]).all() and np.allclose(rows[:, :, c_fac], factors[None, :], rtol=1e-6)
        assert np.allclose(rows[:, :, c_w], 2.0 * factors[None, :], rtol=1e-6) and (rows[:, :, c_mp] > 0).all()
        assert (rows[:KMAX, 0, c_mp].sum() == rows[KMAX, :, c_mp]).all()
        for c in (c_chi2, c_lev):
            tot, parts = rows[KMAX, :, c], rows[:KMAX, :, c]
            assert (np.abs(parts.sum(axis=0) - tot) <= 1e-7 * (np.abs(parts).sum(axis=0) + np.abs(tot))).all(), (s, c)
        if s == 1:
            for p in range(KMAX + 1):
                chi2, reg, dof = rows[p, :, c_chi2], rows[p, :, c_reg:c_reg + nblk].sum(axis=1), rows[p, :, c_dof:c_dof + nblk].sum(axis=1)
                assert (np.diff(chi2) >= -SLACK * chi2.max()).all(), (p, chi2)
                assert (np.diff(reg) <= SLACK * reg.max()).all(), (p, reg)
                assert (np.diff(dof) <= SLACK * dof.max()).all(), (p, dof)
    log = (tmp_path / "sweep" / "para.in_map.log").read_text().splitlines()
    picks = [line for line in log if line.startswith(" map tradeoff sweep")]
    assert len(picks) == 3 * nsw * (KMAX + 1) and picks == [line for line in out.splitlines() if line.startswith(" map tradeoff sweep")]
    for what in ("L-curve corner", "GCV minimum", "evidence maximum"):
        assert sum(what in line for line in picks) == nsw * (KMAX + 1)
    assert sum("all periods" in line for line in picks) == 3 * nsw
    print("\n[measured] " + "\n[measured] ".join(picks))
    names = sorted(n for n in os.listdir(tmp_path / "plain") if n not in files)
    assert "period_phaseV_map.dat" in names and "para.in_map.log" in names and "map_tradeoff.dat" not in names
    assert sorted(n for n in os.listdir(tmp_path / "sweep") if n not in files) == sorted(names + ["map_tradeoff.dat"])
    strip = lambda text: [line for line in text.splitlines() if "time cost" not in line and not line.startswith(" map tradeoff sweep")]
    for n in names:
        a = (tmp_path / "plain" / n).read_bytes().decode(errors="replace")
        b = (tmp_path / "sweep" / n).read_bytes().decode(errors="replace")
        assert strip(a) == strip(b), n


def test_a_tradeoff_of_one_or_two_points_is_refused(tmp_path):
    prog.build()
    import subprocess
    for name, text in prog.inputs(maxiter=1).items():
        (tmp_path / name).write_text(text)
    out = subprocess.run([prog.MAPS, "para.in", "2.0", "2.0", "0", "2"], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert out.returncode != 0 and "tradeoff is 0 or the number of sweep points" in out.stdout, out.stdout + out.stderr
    assert not (tmp_path / "period_phaseV_map.dat").exists()
