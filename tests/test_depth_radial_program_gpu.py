"""-m gpu: SurfDepthFromMaps_amd with radial = 1: Vsv from the Rayleigh maps and Vsh from the Love maps, cell by
cell, tied by the prior of std sigma_hv on Vsh - Vsv.

A 7 x 7 grid with nz = 4, eight Rayleigh phase and eight Love phase periods over 5-40 s.  The true Vsv is the layered profile with a
lateral bump; the true Vsh is 1.04 Vsv at knot 1 in the cells of the western half (i <= 3) and Vsv elsewhere; both have MOD's deepest
knot.  The maps are exact: the Rayleigh segment of dispersion_kernels_typed on Vsv, the Love segment on Vsh.  MOD is the laterally
uniform profile.  Four iterations, smoothing 2, sigma_c 0.01 km/s, sigma_hv 0.2 km/s.
Measured on an MI355X: radial = 1 log rms_c 0.05971 -> 0.00235 -> 0.00042 -> 0.00039 km/s, final model 0.00038 (Rayleigh / Love before
each iteration 0.03888/0.07496, 0.00090/0.00320, 0.00019/0.00056, 0.00017/0.00052); radial = 0 on the same maps 0.05971 -> 0.01625 ->
0.01604 -> 0.01600, final 0.01598: ratio of the final misfits 0.0238.  RMS((Vsh - Vsv) - truth) / RMS(truth) 0.366; mean xi - 1 at the
anomalous knot of the anomalous cells 0.0642 (truth 0.0816); RMS(Vsh - Vsv) from the maps of an isotropic truth 6.4e-4 km/s."""
import os
import subprocess

import numpy as np
import pytest

from tests.bars import within

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
DEPTH = os.path.join(HOST, "SurfDepthFromMaps_amd")
f32 = np.float32

NX = NY = 7
NCELL = (NX - 2) * (NY - 2)
GOXD, GOZD, DV = 26.5, 101.25, 0.25
DEPZ = np.array([0, 6, 15, 30], f32)
NZ = len(DEPZ)
PROF = np.array([3.0, 3.4, 3.8, 4.3])
PERIODS = np.array([5.0, 8.0, 12.0, 16.0, 21.0, 27.0, 33.0, 40.0])
KV = KH = len(PERIODS)
SUBLAYERS, MAXITER = 3.0, 4
KNOT, AMP = 1, 1.04                                  # the anomalous knot and Vsh / Vsv there
ARGS = ("2.0", "1.0", "0.01", "1", "0", "1", "0.2")   # smooth_vs smooth_gcs sigma_c resolution map_sigma radial sigma_hv
# RMS(Vsh - Vsv) recovered from the maps of an isotropic truth: twice the measured 6.374e-4 km/s (tests/bars.py; what the maps' four
# decimals leave, above the 1e-4 the MOD files are written with)
BAR_ISOTROPIC = 1.3e-3


def true_vsv():
    jj, ii = np.meshgrid(np.arange(NY), np.arange(NX), indexing="ij")
    bump = 0.05 * np.sin(np.pi * (ii - 1) / (NX - 3)) * np.sin(np.pi * (jj - 1) / (NY - 3))
    vel = PROF[:, None, None] * (1.0 + bump[None] * np.array([1.0, 1.0, 0.6, 0.0])[:, None, None])
    return np.ascontiguousarray(vel, f32)


def anomalous():
    """[ny][nx]: the columns where Vsh differs from Vsv"""
    return np.broadcast_to(np.arange(NX)[None, :] <= 3, (NY, NX))


def true_vsh(aniso=True):
    vel = true_vsv().copy()
    if aniso:
        vel[KNOT][anomalous()] *= f32(AMP)
    return vel


def para_text(kv=KV, kh=KH, iso=True):
    lines = ["c" * 70, "c INPUT PARAMETERS", "c" * 70, "surf.dat   c: traveltime data file", f"{NX} {NY} {NZ}   c: nx ny nz",
             f"{GOXD} {GOZD}   c: goxd gozd", f"{DV} {DV}   c: dvxd dvzd", f"{SUBLAYERS:g}   c: number of sublayers",
             "2.0 5.0   c: minimum and maximum Vsv", "8   c: max(sources, receivers)", "0.9   c: sparsity fraction",
             f"{MAXITER}   c: maximum of iteration", f"{'T' if iso else 'F'}   c: iso-mode", "cccccccc control parameters",
             "2.0   c: smoothing for dVsv", "1.0   c: smoothing for Gc,s", "0.0   c: damping", "cccccccccc periods"]
    for k, name in ((kv, "kmaxRc"), (0, "kmaxRg"), (kh, "kmaxLc"), (0, "kmaxLg")):
        lines.append(f"{k}   c: {name}")
        if k:
            lines.append(" ".join(f"{x:g}" for x in PERIODS[:k]))
    return "\n".join(lines) + "\n"


def mod_text(vel):
    out = [" ".join(f"{d:.1f}" for d in DEPZ)]
    for k in range(NZ):
        for j in range(NY):
            out.append(" ".join(f"{vel[k, j, i]:.4f}" for i in range(NX)))
    return "\n".join(out) + "\n"


def maps_text(ctx, vsv, vsh):
    """period_phaseV_map.dat of exact curves: lon lat period c wavetp veltp, the Rayleigh periods of vsv, then the Love periods of vsh"""
    out = []
    for vel, iwave in ((vsv, 2), (vsh, 1)):
        pv, _, nf = ctx.dispersion_kernels_typed(vel, DEPZ, [(iwave, 0, PERIODS)], SUBLAYERS, kernels=False)
        assert nf == 0
        c = pv.reshape(len(PERIODS), NY, NX)
        for t, per in enumerate(PERIODS):
            for j in range(1, NY - 1):
                for i in range(1, NX - 1):
                    out.append("%10.4f%10.4f%10.4f%10.4f%3d%3d" % (GOZD + (j - 1) * DV, GOXD - (i - 1) * DV, per, c[t, j, i], iwave, 0))
    return "\n".join(out) + "\n"


def write_inputs(d, maps, para=None):
    d.mkdir(exist_ok=True)
    (d / "para.in").write_text(para_text() if para is None else para)
    (d / "MOD").write_text(mod_text(np.broadcast_to(PROF[:, None, None], (NZ, NY, NX))))
    (d / "period_phaseV_map.dat").write_text(maps)
    return d


def run(d, *args, ok=True):
    out = subprocess.run([DEPTH, "para.in", *args], cwd=d, timeout=300, capture_output=True, text=True)
    if ok:
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.returncode, out.stdout + out.stderr


def read_mod(path):
    lines = path.read_text().splitlines()
    rows = np.array([[float(v) for v in line.split()] for line in lines[1:] if line.strip()])
    assert rows.shape == (NZ * NY, NX)
    return rows.reshape(NZ, NY, NX)


def nlines(path):
    return sum(1 for line in path.read_text().splitlines() if line.strip())


def log_rows(text, nfield):
    """the per-iteration lines of the log (two integers, then nfield - 2 numbers) and the final model's misfit, its first number"""
    rows = [[float(v) for v in f] for f in (line.split() for line in text.splitlines()) if len(f) == nfield and f[0].isdigit() and f[1].isdigit()]
    final = [line.split() for line in text.splitlines() if line.strip().startswith("final model:")]
    assert len(final) == 1 and len(rows) == MAXITER, text
    return np.array(rows), float(final[0][final[0].index("rms_c") + 1])


INNER = (slice(0, NZ - 1), slice(1, -1), slice(1, -1))


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


@pytest.fixture(scope="module")
def built(ctx):
    subprocess.check_call(["make", "-s", "-C", HOST, "all"])
    return ctx


@pytest.fixture(scope="module")
def radial_run(built, tmp_path_factory):
    """the anisotropic truth through radial = 1 with resolution = 1, and through radial = 0 on the same maps"""
    maps = maps_text(built, true_vsv(), true_vsh())
    d = write_inputs(tmp_path_factory.mktemp("radial"), maps)
    run(d, *ARGS)
    d0 = write_inputs(tmp_path_factory.mktemp("iso"), maps)
    run(d0, *ARGS[:5])
    return d, d0


def test_every_file_with_its_lines_and_columns(radial_run):
    d, _ = radial_run
    assert nlines(d / "MOD_2step") == nlines(d / "MOD_Vsh_2step") == 1 + NZ * NY
    inv = np.loadtxt(d / "DSurfTomo_2step.inv", ndmin=2)
    model = np.loadtxt(d / "Vsv_Vsh_model_2step.inv", ndmin=2)
    res = np.loadtxt(d / "Vsv_Vsh_resolution_2step.dat", ndmin=2)
    c = np.loadtxt(d / "period_phaseV_2step.dat", ndmin=2)
    assert inv.shape == (NZ * NY * NX, 4) and model.shape == (NZ * NY * NX, 7) and res.shape == ((NZ - 1) * NCELL, 14)
    assert c.shape == ((KV + KH) * NCELL, 6) and np.array_equal(c[:, 4], np.repeat([2, 1], KV * NCELL))
    vsv, vsh = read_mod(d / "MOD_2step"), read_mod(d / "MOD_Vsh_2step")
    assert np.allclose(inv[:, 3].reshape(NZ, NY, NX), vsv, atol=1e-4) and np.allclose(model[:, :4], inv, atol=1e-4)
    assert np.allclose(model[:, 4].reshape(NZ, NY, NX), vsh, atol=1e-4)
    assert np.allclose(model[:, 5], np.sqrt((2 * model[:, 3] ** 2 + model[:, 4] ** 2) / 3), atol=2e-4)
    assert np.allclose(model[:, 6], (model[:, 4] / model[:, 3]) ** 2, atol=2e-4)
    assert (vsv[-1] == PROF[-1]).all() and (vsh[-1] == PROF[-1]).all()   # MOD's deepest knot
    assert np.allclose(res[:, 3].reshape(NZ - 1, NY - 2, NX - 2), vsv[INNER], atol=1e-4)
    assert "Program finishes successfully" in (d / "para.in_2step.log").read_text()


def test_misfit_falls_and_ends_below_the_isotropic_runs(radial_run):
    d, d0 = radial_run
    rows, final = log_rows((d / "para.in_2step.log").read_text(), 10)
    rows0, final0 = log_rows((d0 / "para.in_2step.log").read_text(), 5)
    seq = list(rows[:, 2]) + [final]
    print("\n[measured] radial = 1 rms_c per iteration and final (km/s): " + " ".join("%.5f" % m for m in seq))
    print("[measured] Rayleigh, Love before each iteration: " + " ".join("%.5f/%.5f" % (a, b) for a, b in rows[:, 4:6]))
    print("[measured] radial = 0 on the same maps: " + " ".join("%.5f" % m for m in list(rows0[:, 2]) + [final0]))
    assert all(b < a for a, b in zip(seq, seq[1:])), seq
    within("final rms_c, radial = 1 / radial = 0", final / final0, 1.0 - 1e-6)
    assert rows[0, 2] == rows0[0, 2]                      # (both start from MOD's curves)


def test_recovers_the_difference_better_than_isotropy_does(radial_run):
    d, _ = radial_run
    diff = (read_mod(d / "MOD_Vsh_2step") - read_mod(d / "MOD_2step"))[INNER]
    truth = (true_vsh().astype(np.float64) - true_vsv())[INNER]
    within("RMS((Vsh - Vsv) - truth) / RMS(truth)", rms(diff - truth) / rms(truth), 1.0 - 1e-6)
    model = np.loadtxt(d / "Vsv_Vsh_model_2step.inv", ndmin=2)
    xi = model[:, 6].reshape(NZ, NY, NX)[KNOT, 1:-1, 1:-1][anomalous()[1:-1, 1:-1]]
    print(f"\n[measured] mean xi - 1 at the anomalous knot of the anomalous cells: {xi.mean() - 1:.4f} (truth {AMP ** 2 - 1:.4f})")
    assert xi.mean() - 1 > 0


def test_isotropic_truth_stays_isotropic(built, tmp_path):
    d = write_inputs(tmp_path, maps_text(built, true_vsv(), true_vsh(aniso=False)))
    run(d, *ARGS)
    diff = (read_mod(d / "MOD_Vsh_2step") - read_mod(d / "MOD_2step"))[INNER]
    within("RMS(Vsh - Vsv) from the maps of an isotropic truth (km/s)", rms(diff), BAR_ISOTROPIC)


def test_refusals_name_their_cause(built, tmp_path):
    maps = maps_text(built, true_vsv(), true_vsh())
    rayleigh_only = "".join(line + "\n" for line in maps.splitlines()[:KV * NCELL])
    for name, para, args, words in (("no_love", para_text(kh=0), ARGS, ("radial", "Love periods")),
                                    ("iso_f", para_text(iso=False), ARGS, ("radial", "iso-mode")),
                                    ("word", para_text(), ARGS[:5] + ("yes",), ("yes",)),
                                    ("two", para_text(), ARGS[:5] + ("2",), ("radial must be 0 or 1",))):
        d = write_inputs(tmp_path / name, rayleigh_only if name == "no_love" else maps, para)
        rc, out = run(d, *args, ok=False)
        assert rc != 0 and all(w in out for w in words) and "Program finishes successfully" not in out, (name, out)
        assert not (d / "MOD_Vsh_2step").exists()


def test_resolution_file_is_a_posterior(radial_run):
    d, _ = radial_run
    res = np.loadtxt(d / "Vsv_Vsh_resolution_2step.dat", ndmin=2)
    xi, sv, sh, corr, sxi = res[:, 5], res[:, 6], res[:, 7], res[:, 8], res[:, 9]
    assert np.isfinite(res).all() and (sv > 0).all() and (sh > 0).all()
    assert (np.abs(corr) <= 1.0 + 1e-5).all() and (sxi >= 0).all() and (xi > 0.5).all()
    assert (corr > 0).any()                               # (the coupling ties the two profiles)
    log = (d / "para.in_2step.log").read_text()
    assert "resolution VsvVsh" in log
