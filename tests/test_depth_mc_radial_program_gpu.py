"""-m gpu: SurfDepthMC_amd with radial = 1: Vsv, Vsh and xi = (Vsh / Vsv)^2 posteriors per cell from the
Rayleigh and Love maps together.

The 7 x 7, nz = 4, 8 + 8-period case of tests/test_depth_radial_program_gpu.py (its generators: the true Vsh is 1.04 Vsv at knot 1 in the
western cells, the maps are exact, MOD is the laterally uniform profile), 200 + 200 steps, 16 chains, width 0.4, proposal 1, sigma_c
0.01, sigma_hv 0.2, one seed.
Measured on an MI355X: the truth's xi inside the printed interval at 75 of 75 (cell, knot)s, the interval's median width 0.200; mean
xi - 1 at the anomalous knot 0.0573 in the anomalous cells (truth 0.0816) and -0.0048 in the others, the median P(xi > 1) there 0.866
against 0.463; R-hat of xi at most 1.222 after these 200 steps."""
import subprocess

import numpy as np
import pytest

from tests.test_depth_radial_program_gpu import (AMP, HOST, INNER, KH, KNOT, KV, NCELL, NX, NY, NZ, anomalous, maps_text, nlines, para_text,
                                                 read_mod, true_vsh, true_vsv, write_inputs)

pytestmark = pytest.mark.gpu
MC = HOST + "/SurfDepthMC_amd"
NLAY = NZ - 1


def mc_args(nsample=200, smooth_vs=0.0, types=1, aniso_thin=0, tail=("1", "0.2")):
    """nsample nchain width sigma_c seed proposal ntemp tmax aniso_thin smooth_gcs sigma_a noise_a0 noise_b0 smooth_vs damp_vs types, then
    `tail`: radial sigma_hv"""
    return (str(nsample), "16", "0.4", "0.01", "1", "1", "1", "16", str(aniso_thin), "1.0", "0.01", "0", "1", f"{smooth_vs:g}", "0",
            str(types)) + tuple(tail)


def run(d, *args, ok=True):
    out = subprocess.run([MC, "para.in", *args], cwd=d, timeout=300, capture_output=True, text=True)
    if ok:
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.returncode, out.stdout + out.stderr


@pytest.fixture(scope="module")
def built(ctx):
    subprocess.check_call(["make", "-s", "-C", HOST, "all"])
    return ctx


@pytest.fixture(scope="module")
def maps(built):
    return maps_text(built, true_vsv(), true_vsh())


@pytest.fixture(scope="module")
def radial_dir(maps, tmp_path_factory):
    d = write_inputs(tmp_path_factory.mktemp("mc_radial"), maps)
    run(d, *mc_args())
    return d


def test_every_file_with_its_lines_and_columns(radial_dir):
    d = radial_dir
    assert nlines(d / "MOD_mc") == nlines(d / "MOD_Vsh_mc") == 1 + NZ * NY
    shapes = {"DSurfTomo_mc.inv": (NZ * NY * NX, 4), "Vs_posterior_mc.dat": (NLAY * NCELL, 10), "Vsh_posterior_mc.dat": (NLAY * NCELL, 10),
              "xi_posterior_mc.dat": (NLAY * NCELL, 13), "Vsv_Vsh_model_mc.inv": (NZ * NY * NX, 7),
              "period_phaseV_mc.dat": ((KV + KH) * NCELL, 6), "cell_mc.dat": (NCELL, 5)}
    f = {name: np.loadtxt(d / name, ndmin=2) for name in shapes}
    for name, shape in shapes.items():
        assert f[name].shape == shape and np.isfinite(f[name]).all(), name
    assert np.array_equal(f["period_phaseV_mc.dat"][:, 4], np.repeat([2, 1], KV * NCELL))
    assert not (d / "Vsv_Vsh_prior_check_mc.dat").exists() and not (d / "noise_posterior_mc.dat").exists()
    vsv, vsh = read_mod(d / "MOD_mc"), read_mod(d / "MOD_Vsh_mc")
    # the MOD files hold the means of the posterior files, to the printed digits; the deepest knot is MOD's in both
    assert np.allclose(f["Vs_posterior_mc.dat"][:, 3].reshape(NLAY, NY - 2, NX - 2), vsv[INNER], atol=1.0001e-4)
    assert np.allclose(f["Vsh_posterior_mc.dat"][:, 3].reshape(NLAY, NY - 2, NX - 2), vsh[INNER], atol=1.0001e-4)
    assert (vsv[-1] == vsv[-1, 0, 0]).all() and np.array_equal(vsv[-1], vsh[-1])
    model = f["Vsv_Vsh_model_mc.inv"]
    assert np.allclose(model[:, 3].reshape(NZ, NY, NX), vsv, atol=1e-4) and np.allclose(model[:, 4].reshape(NZ, NY, NX), vsh, atol=1e-4)
    assert np.allclose(model[:, 5], np.sqrt((2 * model[:, 3] ** 2 + model[:, 4] ** 2) / 3), atol=2e-4)
    # its xi is the posterior mean of xi at the sampled knots, (Vsh / Vsv)^2 of the start model elsewhere
    xi = f["xi_posterior_mc.dat"]
    assert np.allclose(model[:, 6].reshape(NZ, NY, NX)[INNER], xi[:, 3].reshape(NLAY, NY - 2, NX - 2), atol=1.0001e-5)
    assert (model[:, 6].reshape(NZ, NY, NX)[-1] == 1).all() and (model[:, 6].reshape(NZ, NY, NX)[:, 0] == 1).all()
    assert (xi[:, 4] > 0).all() and (xi[:, 5] <= xi[:, 6]).all() and (xi[:, 6] <= xi[:, 7]).all()
    assert ((xi[:, 9] >= 0) & (xi[:, 9] <= 1)).all() and (np.abs(xi[:, 10]) <= 1).all() and (xi[:, 12] > 0).all()
    log = (d / "para.in_mc.log").read_text()
    for words in ("radial anisotropy: Vsv from the", "R-hat of xi over (cell, knot), median and maximum:",
                  "share of sampled (cell, knot)s with P(xi > 1) outside [0.025, 0.975]:", "Program finishes successfully"):
        assert words in log, words


def test_truth_inside_the_interval_and_the_anomaly_found(radial_dir):
    """the truth's xi lies inside the printed [p2.5, p97.5] at every inner cell and knot, and the mean xi - 1 at the anomalous knot of
    the anomalous cells is nearer the truth 0.0816 than 0"""
    xi = np.loadtxt(radial_dir / "xi_posterior_mc.dat", ndmin=2)
    truth = ((true_vsh().astype(np.float64) / true_vsv()) ** 2)[INNER].ravel()
    lo, hi = xi[:, 5], xi[:, 7]
    inside = (lo - 1e-5 <= truth) & (truth <= hi + 1e-5)              # (the file's five decimals)
    west = anomalous()[1:-1, 1:-1]
    mean = xi[:, 3].reshape(NLAY, NY - 2, NX - 2)[KNOT][west].mean() - 1
    print(f"\n[measured] truth inside the printed interval at {inside.sum()} of {inside.size} (cell, knot)s; interval width median "
          f"{np.median(hi - lo):.4f}; mean xi - 1 at the anomalous knot of the anomalous cells {mean:.4f} (truth {AMP ** 2 - 1:.4f}), of the "
          f"other cells {xi[:, 3].reshape(NLAY, NY - 2, NX - 2)[KNOT][~west].mean() - 1:.4f}; P(xi > 1) there median "
          f"{np.median(xi[:, 9].reshape(NLAY, NY - 2, NX - 2)[KNOT][west]):.3f} against "
          f"{np.median(xi[:, 9].reshape(NLAY, NY - 2, NX - 2)[KNOT][~west]):.3f}; R-hat of xi max {xi[:, 8].max():.3f}")
    assert inside.all(), np.argwhere(~inside.reshape(NLAY, NY - 2, NX - 2))
    assert abs(mean - (AMP ** 2 - 1)) < abs(mean)


def test_prior_check_file(maps, tmp_path):
    """smooth_vs > 0 with noise_a0 = 0 adds Vsv_Vsh_prior_check_mc.dat: the chains' stds beside the linearised ones, with their ratios"""
    d = write_inputs(tmp_path, maps)
    run(d, *mc_args(nsample=60, smooth_vs=2.0))
    chk = np.loadtxt(d / "Vsv_Vsh_prior_check_mc.dat", ndmin=2)
    assert chk.shape == (NLAY * NCELL, 9) and np.isfinite(chk).all() and (chk[:, 3:] > 0).all()
    assert np.allclose(chk[:, 5], chk[:, 3] / chk[:, 4], rtol=1e-3) and np.allclose(chk[:, 8], chk[:, 6] / chk[:, 7], rtol=1e-3)
    log = (d / "para.in_mc.log").read_text()
    assert "std / linearised std of Vsv" in log and "std / linearised std of Vsh" in log


def test_radial_0_writes_the_bytes_of_the_run_without_it(maps, tmp_path):
    d = write_inputs(tmp_path, maps)
    out = {}
    for name, tail in (("without", ()), ("zero", ("0",)), ("zero_sigma", ("0", "0.5"))):
        run(d, *mc_args(nsample=40, tail=tail))
        files = sorted(p.name for p in d.iterdir() if p.name.endswith(("_mc", "_mc.dat", "_mc.inv", "_mc.log")))
        # (the run's seconds are the one line of the log that differs between any two runs)
        out[name] = {f: b"\n".join(line for line in (d / f).read_bytes().split(b"\n") if not line.startswith(b" run ")) for f in files}
        assert "MOD_Vsh_mc" not in files and "xi_posterior_mc.dat" not in files and "Vs_posterior_mc.dat" in files
    assert out["without"] == out["zero"] == out["zero_sigma"]


def test_refusals_name_their_cause(maps, tmp_path):
    rayleigh_only = "".join(line + "\n" for line in maps.splitlines()[:KV * NCELL])
    love_only = "".join(line + "\n" for line in maps.splitlines()[KV * NCELL:])
    deep = para_text().replace(f"{NX} {NY} {NZ}   c: nx ny nz", f"{NX} {NY} 33   c: nx ny nz")
    for name, para, text, args, words in (
            ("types_0", para_text(kh=0), rayleigh_only, mc_args(types=0), ("radial = 1", "types = 1")),
            ("no_love", para_text(kh=0), rayleigh_only, mc_args(), ("radial = 1", "Love periods")),
            ("no_rayleigh", para_text(kv=0), love_only, mc_args(), ("radial = 1", "Rayleigh periods")),
            ("aniso", para_text(iso=False), maps, mc_args(aniso_thin=5), ("aniso_thin",)),
            ("deep", deep, maps, mc_args(), ("radial = 1", "nz - 1 <= 31")),
            ("two", para_text(), maps, mc_args(tail=("2",)), ("radial must be 0 or 1",)),
            ("sigma", para_text(), maps, mc_args(tail=("1", "-0.1")), ("sigma_hv",))):
        d = write_inputs(tmp_path / name, text, para)
        rc, out = run(d, *args, ok=False)
        assert rc != 0 and all(w in out for w in words) and "Program finishes successfully" not in out, (name, out)
        assert not (d / "MOD_mc").exists() and not (d / "MOD_Vsh_mc").exists()
