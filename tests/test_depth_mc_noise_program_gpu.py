"""-m gpu: SurfDepthMC_amd with the hierarchical noise scale (arguments 13 and 14: noise_a0, noise_b0) on the test1 fixtures of
test_depth_mc_program_gpu.py."""
import numpy as np
import pytest

from tests.test_depth_from_maps_gpu import NX, NY
from tests.test_depth_mc_program_gpu import MC, OUTS, run_failing, true_knot_files
from tests.test_phase_map_program_gpu import build, run

pytestmark = pytest.mark.gpu

# nsample nchain width sigma_c seed proposal ntemp tmax aniso_thin smooth_gcs sigma_a: the defaults, spelled out
BASE = ("30", "4", "0", "0.01", "7", "0", "1", "16", "0", "0", "0.01")
NOISE_FILE = "noise_posterior_mc.dat"


def test_noise_off_is_the_program_as_it_was(tmp_path):
    """noise_a0 = 0 given as an argument: every file and the log equal those of a run without arguments 13 and 14, byte for byte
    apart from the log's timing line, and no noise file is written"""
    build()
    files, _, _ = true_knot_files()
    got = {}
    for name, extra in (("without", ()), ("zero", ("0", "0"))):
        out = run(MC, tmp_path / name, files, *BASE, *extra)
        assert "Program finishes successfully" in out
        assert not (tmp_path / name / NOISE_FILE).exists()
        got[name] = {n: (tmp_path / name / n).read_bytes() for n in OUTS if n != "para.in_mc.log"}
        log = (tmp_path / name / "para.in_mc.log").read_text()
        assert "hierarchical noise" not in log and "noise scale over cells" not in log
        got[name]["log"] = [ln for ln in log.splitlines() if not ln.startswith(" run ")]
    assert got["without"] == got["zero"]


def test_noise_on(tmp_path):
    """noise_a0 2, noise_b0 1: the file's shape and content, the two log keys, and equal bytes from two runs with one seed"""
    build()
    files, _, _ = true_knot_files()
    ncell = (NX - 2) * (NY - 2)
    got = []
    for name in ("a", "b"):
        out = run(MC, tmp_path / name, files, *BASE, "2", "1")
        assert "Program finishes successfully" in out
        got.append({n: (tmp_path / name / n).read_bytes() for n in OUTS + (NOISE_FILE,) if n != "para.in_mc.log"})
    assert got[0] == got[1]
    post = np.loadtxt(tmp_path / "a" / NOISE_FILE, ndmin=2)
    assert post.shape == (ncell, 6)
    cells = np.loadtxt(tmp_path / "a" / "cell_mc.dat", ndmin=2)
    assert np.array_equal(post[:, :2], cells[:, :2])          # lon, lat of the same inner cells
    sampled = post[:, 5] > 0
    assert sampled.any() and np.isfinite(post[sampled, 2]).all() and (post[sampled, 2] > 0).all()
    assert (post[~sampled, 2:5] == 0).all()
    # column 5 = sigma_c * column 3, both printed with six decimals
    assert np.abs(post[:, 4] - 0.01 * post[:, 2]).max() <= 0.5e-6 * (1 + 0.01) + 1e-9
    log = (tmp_path / "a" / "para.in_mc.log").read_text()
    for key in ("hierarchical noise", "noise scale over cells"):
        assert key in log, key
    plain = tmp_path / "plain"
    run(MC, plain, files, *BASE)
    assert (plain / "Vs_posterior_mc.dat").read_bytes() != got[0]["Vs_posterior_mc.dat"]
    print(f"\n[measured] lam_mean over sampled cells {post[sampled, 2].min():.3f}..{post[sampled, 2].max():.3f}, median "
          f"{np.median(post[sampled, 2]):.3f}; periods per cell {int(post[sampled, 5].min())}..{int(post[:, 5].max())}")


def test_bad_noise_arguments_stop_with_a_message(tmp_path):
    build()
    files, _, _ = true_knot_files()
    for name, extra, msg in (("a0", ("-1", "1"), "noise_a0 must not be negative"), ("b0", ("2", "0"), "noise_b0 must be positive"),
                             ("b0neg", ("2", "-3"), "noise_b0 must be positive")):
        rc, text = run_failing(tmp_path / name, files, *BASE, *extra)
        assert rc != 0 and msg in text, (name, text)
        assert not (tmp_path / name / "MOD_mc").exists(), name
        assert not (tmp_path / name / NOISE_FILE).exists(), name
