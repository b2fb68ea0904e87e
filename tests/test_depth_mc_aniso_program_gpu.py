"""-m gpu: the program SurfDepthMC_amd with its aniso_thin, smooth_gcs and sigma_a arguments (Gc/Gs posteriors from the Vs chains,
DESIGN.md section 14) on the fixtures of test_depth_mc_program_gpu.py: test1's true maps, iso-mode F, a short run."""
import numpy as np
import pytest

import dazimsurftomo_amd as dz
from tests.test_depth_from_maps_gpu import NX, NY, NZ, nlines, read_mod_text
from tests.test_depth_mc_program_gpu import MC, OUTS, run_failing, true_knot_files
from tests.test_phase_map_program_gpu import KMAX, build, inputs, run

pytestmark = pytest.mark.gpu

NEW = ("Gc_Gs_posterior_mc.dat", "Gc_Gs_model_mc.inv")
ARGS = ("30", "4", "0", "0.01", "7", "0", "1", "16")          # nsample nchain width sigma_c seed proposal ntemp tmax
LOG_KEYS = ("Gc/Gs posteriors: one sample", "Gc/Gs passes", "std_between / std")


def iso_f_files():
    files, _, _ = true_knot_files()
    files["para.in"] = inputs(maxiter=3, iso="F")["para.in"]
    assert "period_Azm_tomo_map.inv" in files
    return files


def mirror_result(files, nsample, nchain, seed, nthin):
    """what the program computes, through the Python mirror on the same inputs: MOD as vel0, para.in's Vs range as the box, column 4
    of period_phaseV_map.dat and columns 8, 9 of period_Azm_tomo_map.inv, weight 1/sigma everywhere (no coverage file), para.in's
    Gc/Gs smoothing 2.0 and damping 0.0, step 0.05, adaptation every 50, 200 bins"""
    sh = (KMAX, NY - 2, NX - 2)
    vel0 = read_mod_text(files["MOD"]).astype(np.float32)
    depz = np.array(files["MOD"].splitlines()[0].split(), np.float32)
    periods = np.array([5.0, 12.0, 25.0, 40.0])
    c = np.array([l.split() for l in files["period_phaseV_map.dat"].splitlines() if l.strip()], np.float64)
    a = np.array([l.split() for l in files["period_Azm_tomo_map.inv"].splitlines() if l.strip()], np.float64)
    cmap = c[:, 3].astype(np.float32).reshape(sh)
    amap = np.stack([a[:, 7].astype(np.float32).reshape(sh), a[:, 8].astype(np.float32).reshape(sh)])
    w = np.full(sh, np.float32(1.0) / np.float32(0.01), np.float32)
    vmin = np.full((NZ - 1, NY - 2, NX - 2), 2.0, np.float32)
    vmax = np.full((NZ - 1, NY - 2, NX - 2), 4.8, np.float32)
    ctx = dz.Context(0)
    mc = ctx.mc_create(NX, NY, NZ, KMAX, nchain, 200, seed, vel0, vmin, vmax, cmap, w, 0.05, 50,
                       aniso=dict(nthin=nthin, amap=amap, wa=w, smooth=2.0, damp=0.0))
    mc.run(depz, 2.0, periods, nsample, nsample)
    r = mc.aniso_result()
    mc.free()
    ctx.close()
    return r


def test_aniso_thin_adds_two_files_and_changes_no_other(tmp_path):
    build()
    files = iso_f_files()
    out0 = run(MC, tmp_path / "off", files, *ARGS, "0")
    assert not any((tmp_path / "off" / n).exists() for n in NEW)
    assert not any(k in out0 for k in LOG_KEYS)
    out5 = run(MC, tmp_path / "on", files, *ARGS, "5")
    assert all((tmp_path / "on" / n).exists() for n in NEW)
    log = (tmp_path / "on" / "para.in_mc.log").read_text()
    for k in LOG_KEYS + ("read period_Azm_tomo_map.inv",):
        assert k in log and k in out5, k
    for n in OUTS:
        if n != "para.in_mc.log":
            assert (tmp_path / "on" / n).read_bytes() == (tmp_path / "off" / n).read_bytes(), n
    # a run without the argument is the aniso_thin 0 run
    run(MC, tmp_path / "default", files, *ARGS)
    for n in OUTS:
        if n != "para.in_mc.log":
            assert (tmp_path / "default" / n).read_bytes() == (tmp_path / "off" / n).read_bytes(), n
    assert not any((tmp_path / "default" / n).exists() for n in NEW)
    ncell = (NX - 2) * (NY - 2)
    post = np.genfromtxt(tmp_path / "on" / "Gc_Gs_posterior_mc.dat")
    assert post.shape == ((NZ - 1) * ncell, 14)
    assert nlines(tmp_path / "on" / "Gc_Gs_model_mc.inv") == (NZ - 1) * ncell
    # the file's counts, means and stds are dazim_mc_aniso_result's to the printed digit (f12.6)
    r = mirror_result(files, 30, 4, 7, 5)
    shp = (NZ - 1, NY - 2, NX - 2)
    assert np.array_equal(post[:, 13].reshape(shp), np.broadcast_to(r["nsamp"], shp))
    assert r["nsamp"].max() == 6 * 4                          # 30 recorded steps, every fifth, 4 chains
    line = [l for l in log.splitlines() if "Gc/Gs passes" in l][0].split()
    assert line[2] == "6" and int(line[5]) == 6 * 4 * ncell - int(r["nsamp"].sum())
    cols = {3: r["mean"][0], 4: r["std"][0], 5: r["mean"][1], 6: r["std"][1], 7: r["std_between"][0], 8: r["std_between"][1]}
    for cidx, v in cols.items():
        assert np.abs(post[:, cidx].reshape(shp) - v.astype(np.float64)).max() <= 0.5000001e-6, cidx
    assert (post[:, 4] > 0).all() and (post[:, 6] > 0).all() and (post[:, 7] <= post[:, 4] + 1e-6).all()
    # amplitude and axis from the printed means, as write_azimuthal forms them
    gc, gs = post[:, 3], post[:, 5]
    assert np.allclose(post[:, 9], 0.5 * np.hypot(gc, gs), atol=2e-6)
    ang = 0.5 * (np.degrees(np.arctan2(gs, gc)) % 360.0)
    d = np.abs(post[:, 11] - ang)
    big = post[:, 9] > 1e-3                                     # (the printed means carry six decimals)
    assert big.any() and np.minimum(d, 180.0 - d)[big].max() <= 0.5
    model = np.loadtxt(tmp_path / "on" / "Gc_Gs_model_mc.inv", ndmin=2)
    assert model.shape[1] == 8 and np.allclose(model[:, 6], 100 * gc, atol=1e-3)
    share = float([l for l in log.splitlines() if "std_between / std" in l][0].split(":")[-1])
    print(f"\n[measured] median std_between / std {share:.4f}; median Gc std {np.median(post[:, 4]):.5f}")
    assert 0 <= share <= 1


def test_iso_mode_t_is_refused(tmp_path):
    build()
    files, _, _ = true_knot_files()
    rc, text = run_failing(tmp_path / "iso", files, *ARGS, "5")
    assert rc != 0 and "aniso_thin > 0 needs the 2-psi maps of iso-mode F" in text
    assert not (tmp_path / "iso" / "MOD_mc").exists()
    rc, text = run_failing(tmp_path / "neg", dict(files, **{"para.in": inputs(maxiter=3, iso="F")["para.in"]}), *ARGS, "-1")
    assert rc != 0 and "aniso_thin must not be negative" in text
