"""-m gpu: SurfDepthMC_amd with the Gaussian smoothness prior (arguments 15 and 16: smooth_vs, damp_vs) on the test1 fixtures of
test_depth_mc_program_gpu.py."""
import numpy as np
import pytest

from tests.test_depth_from_maps_gpu import NX, NY
from tests.test_depth_mc_program_gpu import MC, OUTS, run_failing, true_knot_files
from tests.test_phase_map_program_gpu import build, run

pytestmark = pytest.mark.gpu

# nsample nchain width sigma_c seed proposal ntemp tmax aniso_thin smooth_gcs sigma_a noise_a0 noise_b0: the defaults, spelled out
BASE = ("30", "4", "0", "0.01", "7", "0", "1", "16", "0", "0", "0.01", "0", "1")
CHECK_FILE = "Vs_prior_check_mc.dat"
SETTINGS, SUMMARY = "Gaussian prior about MOD", "Gaussian prior: chains' std / linearised std_post"


def test_prior_off_is_the_program_as_it_was(tmp_path):
    """smooth_vs = damp_vs = 0 given as arguments: every file and the log equal those of a run without arguments 15 and 16, byte for
    byte apart from the log's timing line, and no check file is written"""
    build()
    files, _, _ = true_knot_files()
    got = {}
    for name, extra in (("without", ()), ("zero", ("0", "0"))):
        out = run(MC, tmp_path / name, files, *BASE, *extra)
        assert "Program finishes successfully" in out
        assert not (tmp_path / name / CHECK_FILE).exists()
        got[name] = {n: (tmp_path / name / n).read_bytes() for n in OUTS if n != "para.in_mc.log"}
        log = (tmp_path / name / "para.in_mc.log").read_text()
        assert "Gaussian prior" not in log
        got[name]["log"] = [ln for ln in log.splitlines() if not ln.startswith(" run ")]
    assert got["without"] == got["zero"]


def test_prior_on(tmp_path):
    """smooth_vs 2, damp_vs 1: the settings and the summary line, one line of the check file per inner cell and sampled knot with
    finite values where the cell is sampled and the ratio = std / std_post, other chains than without the prior; with the noise scale
    on the file is not written and the log says why"""
    build()
    files, _, _ = true_knot_files()
    ncell = (NX - 2) * (NY - 2)
    out = run(MC, tmp_path / "on", files, *BASE, "2", "1")
    assert "Program finishes successfully" in out
    log = (tmp_path / "on" / "para.in_mc.log").read_text()
    for key in (SETTINGS, SUMMARY):
        assert key in log and key in out, key
    post = np.loadtxt(tmp_path / "on" / "Vs_posterior_mc.dat", ndmin=2)
    chk = np.loadtxt(tmp_path / "on" / CHECK_FILE, ndmin=2)
    nlay = post.shape[0] // ncell
    assert chk.shape == (nlay * ncell, 6)
    assert np.array_equal(chk[:, :3], post[:, :3])            # lon, lat, depth of the same cells and knots
    sampled = post[:, 4] > 0                                  # (the chains' std: 0 only where nothing was sampled)
    assert sampled.any() and np.isfinite(chk).all()
    assert (chk[sampled, 3] > 0).all() and (chk[sampled, 4] > 0).all() and (chk[sampled, 5] > 0).all()
    assert (chk[~sampled, 3:] == 0).all()
    # column 4 = the posterior file's std (four decimals there, six here); column 6 = column 4 / column 5 of the unrounded values
    assert np.abs(chk[:, 3] - post[:, 4]).max() <= 0.5e-4 + 1e-9
    rel = np.abs(chk[sampled, 5] * chk[sampled, 4] / chk[sampled, 3] - 1)
    assert rel.max() <= 2 * (0.5e-6 / chk[sampled, 3].min() + 0.5e-6 / chk[sampled, 4].min() + 0.5e-5 / chk[sampled, 5].min())
    plain = tmp_path / "plain"
    run(MC, plain, files, *BASE)
    assert (plain / "Vs_posterior_mc.dat").read_bytes() != (tmp_path / "on" / "Vs_posterior_mc.dat").read_bytes()
    line = [ln for ln in log.splitlines() if SUMMARY in ln][0]
    print(f"\n[measured]{line}; ratio over sampled (cell, knot) {chk[sampled, 5].min():.3f}..{chk[sampled, 5].max():.3f}")
    # with the noise scale unknown
    base = BASE[:11] + ("2", "1")
    out = run(MC, tmp_path / "noise", files, *base, "2", "1")
    assert "Program finishes successfully" in out
    assert not (tmp_path / "noise" / CHECK_FILE).exists()
    log = (tmp_path / "noise" / "para.in_mc.log").read_text()
    assert SETTINGS in log and "Vs_prior_check_mc.dat is not written" in log and SUMMARY not in log


def test_bad_prior_arguments_stop_with_a_message(tmp_path):
    build()
    files, _, _ = true_knot_files()
    for name, extra, msg in (("smooth", ("-1", "1"), "smooth_vs must be finite and not negative"),
                             ("damp", ("2", "-0.5"), "damp_vs must be finite and not negative"),
                             ("inf", ("Infinity", "0"), "smooth_vs must be finite and not negative"),
                             ("nan", ("1", "NaN"), "damp_vs must be finite and not negative")):
        rc, text = run_failing(tmp_path / name, files, *BASE, *extra)
        assert rc != 0 and msg in text, (name, text)
        assert not (tmp_path / name / "MOD_mc").exists(), name
        assert not (tmp_path / name / CHECK_FILE).exists(), name
