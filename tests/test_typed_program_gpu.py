"""-m gpu: the host programs on typed surface-wave data (Rayleigh / Love, phase / group velocities in one data file; para.in with
DSurfTomo's kmaxRg / kmaxLc / kmaxLg blocks).

The data come from a "true" model -- the common shape of tests/typed_kernels_ref.py widened to 7 x 7 columns so that rays cross
cells -- through the Python mirror: typed dispersion tables -> eikonal fields -> ray times, written as velocities for all four
types.  Checks:
  a. Rayleigh-phase input with `0 / 0 / 0` lines appended to para.in: every output file of DAzimSurfTomo_amd (iso), SurfPhaseMaps_amd
     and SurfDepthFromMaps_amd is byte-identical to the run without those lines (logs carry run times and are left out);
  b. mixed input through DAzimSurfTomo_amd in iso mode, 2 iterations: m, n and nnz of iteration 1 in the log equal the mirror's, the
     model after iteration 1 equals the mirror's step within the bar tests/test_host_program_gpu.py uses for that comparison
     (LOOP_VS + 1e-3, IterVel.out's three decimals), the weighted residual RMS falls, the model ends nearer the true one than MOD;
  c. the same data through SurfPhaseMaps_amd, then SurfDepthFromMaps_amd: one map per virtual period with the two type columns,
     depth Vs nearer the true model than MOD;
  d. joint mode, SurfDepthMC_amd and a depth run with 61 periods stop with their messages."""
import os
import subprocess

import numpy as np
import pytest

from tests import synth
from tests import typed_kernels_ref as T
from tests.bars import within
from tests.test_host_program_gpu import LOOP_VS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
f32 = np.float32

NX = NY = 7
GOXD, GOZD, DV = 26.5, 101.25, 0.25
NSTA, NSRC = 8, 4
PROF = np.array([3.0, 3.3, 3.6, 3.9, 4.3])
MINVEL, MAXVEL, WEIGHT_VS, DAMP = 2.0, 5.0, 2.0, 0.0
TYPES = [T.RC, T.RG, T.LC, T.LG]                     # para.in's order; (iwave, igr) = the data file's (wavetp, veltp)
OFF, K = T.offsets(T.SEGMENTS)


def true_model():
    jj, ii = np.meshgrid(np.arange(NY), np.arange(NX), indexing="ij")
    bump = 0.05 * np.sin(np.pi * (ii - 1) / (NX - 3)) * np.sin(np.pi * (jj - 1) / (NY - 3))
    vel = PROF[:, None, None] * (1.0 + bump[None] * np.array([1.0, 1.0, 0.6, 0.3, 0.0])[:, None, None])
    return np.ascontiguousarray(vel, f32)


def start_model():
    return np.ascontiguousarray(np.broadcast_to(PROF[:, None, None], (len(PROF), NY, NX)), f32)


def para_text(iso=True, maxiter=2, segments=T.SEGMENTS, extra=""):
    by_type = {(iw, ig): t for iw, ig, t in segments}
    lines = ["c" * 70, "c INPUT PARAMETERS", "c" * 70, "surf_typed.dat   c: traveltime data file", f"{NX} {NY} {len(PROF)}   c: nx ny nz",
             f"{GOXD} {GOZD}   c: goxd gozd", f"{DV} {DV}   c: dvxd dvzd", f"{T.SUBLAYERS:g}   c: number of sublayers",
             f"{MINVEL} {MAXVEL}   c: minimum and maximum Vsv", f"{NSTA}   c: max(sources, receivers)", "0.9   c: sparsity fraction",
             f"{maxiter}   c: maximum of iteration", f"{'T' if iso else 'F'}   c: iso-mode", "cccccccc control parameters",
             f"{WEIGHT_VS}   c: smoothing for dVsv", "1.0   c: smoothing for Gc,s", f"{DAMP}   c: damping", "cccccccccc periods"]
    for key, name in zip(TYPES, ("kmaxRc", "kmaxRg", "kmaxLc", "kmaxLg")):
        t = by_type.get(key, [])
        lines.append(f"{len(t)}   c: {name}")
        if len(t):
            lines.append(" ".join(f"{x:g}" for x in t))
    return "\n".join(lines) + "\n" + extra


def mod_text(vel):
    out = [" ".join(f"{d:.1f}" for d in T.DEPZ)]
    for k in range(vel.shape[0]):
        for j in range(NY):
            out.append(" ".join(f"{vel[k, j, i]:.4f}" for i in range(NX)))
    return "\n".join(out) + "\n"


def great_circle(colat1, lon1, colat2, lon2):
    """host/dazim_io.f90's great_circle in fp32"""
    half, two = f32(0.5), f32(2.0)
    pi = f32(3.1415926535898)
    dlat, dlon = colat2 - colat1, lon2 - lon1
    lat1, lat2 = pi / two - colat1, pi / two - colat2
    a = np.sin(dlat * half) * np.sin(dlat * half) + np.sin(dlon * half) * np.sin(dlon * half) * np.cos(lat1) * np.cos(lat2)
    return (f32(6371.0) * (two * np.arctan2(np.sqrt(a), np.sqrt(f32(1.0) - a)))).astype(f32)


class Survey:
    """stations, and the (virtual period, source, receiver) lists in the data file's order"""

    def __init__(self, kmax=K):
        self.lat, self.lon = synth.stations(NX, NY, GOXD, GOZD, DV, DV, NSTA, seed=11, shrink=0.08)
        self.lat, self.lon = (np.array([float(f"{v:.4f}") for v in a], f32) for a in (self.lat, self.lon))   # the file's four decimals
        sx, sz = synth.radians(self.lat, self.lon)
        self.src, self.rcv = [], []
        for k in range(kmax):
            for s in range(NSRC):
                self.src.append((k, s))
                self.rcv.append([r for r in range(NSTA) if r != s])
        self.scx = np.array([sx[s] for _, s in self.src], f32)
        self.scz = np.array([sz[s] for _, s in self.src], f32)
        self.per = np.array([k + 1 for k, _ in self.src], np.int32)
        self.ray_f = np.array([f for f, rs in enumerate(self.rcv) for _ in rs], np.int32)
        ridx = np.array([r for rs in self.rcv for r in rs])
        self.rcx, self.rcz = sx[ridx].astype(f32), sz[ridx].astype(f32)
        self.dist = great_circle(self.scx[self.ray_f], self.scz[self.ray_f], self.rcx, self.rcz)
        self.ridx = ridx

    def rows(self, ctx, vel, segments, kernels=True):
        """typed tables -> eikonal fields -> (G or None, predicted times)"""
        geo = (NX, NY, GOXD, GOZD, DV, DV)
        pv, sen, nf = ctx.dispersion_kernels_typed(vel, T.DEPZ, segments, T.SUBLAYERS)
        assert nf == 0
        fields = ctx.fmm_batch(*geo, pv, self.scx, self.scz, self.per)
        G, tpred, _ = ctx.rays_build_G(*geo, vel, fields, self.scx, self.scz, self.per, self.ray_f, self.rcx, self.rcz, sen)
        return G, tpred

    def data_text(self, tpred, segments):
        """'# lat lon period wavetp veltp' per source, 'lat lon velocity' per receiver; the period counts within its type"""
        off, _ = T.offsets(segments)
        out, i = [], 0
        for f, (k, s) in enumerate(self.src):
            seg = max(q for q in range(len(segments)) if off[q] <= k)
            iw, ig, _ = segments[seg]
            out.append(f"# {self.lat[s]:9.4f} {self.lon[s]:9.4f} {k - off[seg] + 1} {iw} {ig}")
            for r in self.rcv[f]:
                out.append(f"  {self.lat[r]:9.4f} {self.lon[r]:9.4f} {self.dist[i] / tpred[i]:8.4f}")
                i += 1
        return "\n".join(out) + "\n"


def run(exe, cwd, *args, ok=True):
    out = subprocess.run([os.path.join(HOST, exe), "para.in", *map(str, args)], cwd=cwd, timeout=300, capture_output=True, text=True)
    if ok:
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout + out.stderr


@pytest.fixture(scope="module")
def built(ctx):
    subprocess.check_call(["make", "-s", "-C", HOST, "all"])
    return ctx


@pytest.fixture(scope="module")
def typed_case(built):
    """the survey, the true model and the data file's text (all four types)"""
    sv = Survey()
    G, tpred = sv.rows(built, true_model(), T.SEGMENTS)
    G.free()
    return sv, sv.data_text(tpred, T.SEGMENTS)


def write_inputs(d, para, data, mod=None):
    d.mkdir(exist_ok=True)
    (d / "para.in").write_text(para)
    (d / "surf_typed.dat").write_text(data)
    (d / "MOD").write_text(mod_text(start_model()) if mod is None else mod)
    return d


def iter_vel(d, nz=len(PROF)):
    blocks, cur = [], None
    for ln in open(d / "IterVel.out").read().split("\n"):
        if "OUTPUT S VELOCITY" in ln:
            cur = []
            blocks.append(cur)
        elif "OUTPUT DWS" in ln:
            cur = []
        elif ln.strip():
            cur.extend(float(v) for v in ln.split())
    return [np.array(b).reshape(nz, NY, NX) for b in blocks]


def test_rayleigh_phase_input_with_zero_blocks_keeps_every_output_byte(built, tmp_path):
    rc_only = T.SEGMENTS[:1]
    sv = Survey(len(rc_only[0][2]))
    G, tpred = sv.rows(built, true_model(), rc_only)
    G.free()
    data = sv.data_text(tpred, rc_only)
    plain = para_text(segments=rc_only)
    base = plain[:plain.index("0   c: kmaxRg")]                   # para.in as it always was: ends with the Rayleigh phase periods
    dirs = [write_inputs(tmp_path / "a", base, data), write_inputs(tmp_path / "b", plain, data)]
    for d in dirs:
        run("DAzimSurfTomo_amd", d)
        run("SurfPhaseMaps_amd", d)
        run("SurfDepthFromMaps_amd", d)
    names = sorted(f for f in os.listdir(dirs[0]) if not f.endswith(".log") and f != "para.in")
    assert names == sorted(f for f in os.listdir(dirs[1]) if not f.endswith(".log") and f != "para.in")
    assert {"DSurfTomo.inv", "IterVel.out", "phaseV_FWD.dat", "Traveltime_statis_00th.dat", "period_phaseV_map.dat", "DSurfTomo_2step.inv"} <= set(names)
    for f in names:
        assert open(dirs[0] / f, "rb").read() == open(dirs[1] / f, "rb").read(), f
    assert np.loadtxt(dirs[1] / "phaseV_FWD.dat").shape[1] == 4   # no type columns


def test_mixed_input_through_the_inversion_program(built, typed_case, tmp_path):
    ctx = built
    sv, data = typed_case
    d = write_inputs(tmp_path / "inv", para_text(), data)
    stdout = run("DAzimSurfTomo_amd", d)
    assert "Program finishes successfully" in stdout
    log = open(d / "para.in_inv.log").read()
    # ---- the mirror's first iteration ----
    vs = start_model()
    G, tpred = sv.rows(ctx, vs, T.SEGMENTS)
    obst = (sv.dist / np.array([float(ln.split()[2]) for ln in data.splitlines() if not ln.startswith("#")], f32)).astype(f32)
    res, wgt, rhs, st = ctx.weight_data(G, obst, tpred)
    maxvp = (NX - 2) * (NY - 2) * (len(PROF) - 1)
    G.append_tikhonov(NX, NY, len(PROF), [WEIGHT_VS])
    m, n, nnz = G.m, G.n, G.nnz
    dv, info = ctx.lsmr(G, np.concatenate([rhs, np.zeros(G.m - len(rhs), f32)]), DAMP, 1e-3, 1e-3, 1200, 1000, n // 4)
    G.free()
    ctx.model_update(vs, dv, MINVEL, MAXVEL, False)
    sizes = [ln for ln in log.splitlines() if "[G; L] rows m" in ln]
    assert len(sizes) == 2
    got = [int(x) for x in sizes[0].replace("=", " ").split() if x.isdigit()]
    assert got == [m, n, nnz] and n == maxvp and m == len(obst) + maxvp, (sizes[0], m, n, nnz)
    models = iter_vel(d)
    assert len(models) == 2
    within("typed iso program Vs after iteration 1 vs the mirror's step (3 decimals)", np.abs(models[0] - vs).max(), LOOP_VS + 1e-3)
    assert np.abs(models[0] - start_model()).max() > 0.02          # (a step was taken)
    rms = [float(ln.split()[-2]) for ln in log.splitlines() if "Before Inversion" in ln]
    after = [float(ln.split()[-2]) for ln in log.splitlines() if "After Inversion" in ln]
    assert len(rms) == 2 and rms[1] < rms[0] and after[-1] < rms[0], (rms, after)
    final = np.loadtxt(d / "DSurfTomo.inv")[:, 3].reshape(len(PROF), NY, NX)
    inner = (slice(0, len(PROF) - 1), slice(1, -1), slice(1, -1))
    e0 = np.sqrt(np.mean((start_model()[inner] - true_model()[inner]) ** 2))
    e1 = np.sqrt(np.mean((final[inner] - true_model()[inner]) ** 2))
    print(f"\n[typed inversion] rms before iterations {rms}, model error {e0:.4f} -> {e1:.4f} km/s")
    assert e1 < e0
    # the writers' type columns
    fwd = np.loadtxt(d / "phaseV_FWD.dat")
    assert fwd.shape == (K * (NX - 2) * (NY - 2), 6)
    tt = np.loadtxt(d / "Traveltime_statis_00th.dat", skiprows=1)
    assert tt.shape == (len(obst), 8)
    want = np.repeat([[iw, ig] for iw, ig, t in T.SEGMENTS for _ in t], NSRC * (NSTA - 1), axis=0)
    assert np.array_equal(tt[:, 6:], want)


def test_mixed_input_through_the_maps_and_the_depth_program(built, typed_case, tmp_path):
    sv, data = typed_case
    d = write_inputs(tmp_path / "maps", para_text(maxiter=3), data)
    run("SurfPhaseMaps_amd", d)
    maps = np.loadtxt(d / "period_phaseV_map.dat")
    ncell = (NX - 2) * (NY - 2)
    assert maps.shape == (K * ncell, 6)
    periods = np.concatenate([t for _, _, t in T.SEGMENTS])
    types = np.array([[iw, ig] for iw, ig, t in T.SEGMENTS for _ in t])
    assert np.allclose(maps[::ncell, 2], periods) and np.array_equal(maps[:, 4:], np.repeat(types, ncell, axis=0))
    assert np.isfinite(maps).all() and (maps[:, 3] > 2.0).all()
    run("SurfDepthFromMaps_amd", d)
    final = np.loadtxt(d / "DSurfTomo_2step.inv")[:, 3].reshape(len(PROF), NY, NX)
    inner = (slice(0, len(PROF) - 1), slice(1, -1), slice(1, -1))
    e0 = np.sqrt(np.mean((start_model()[inner] - true_model()[inner]) ** 2))
    e1 = np.sqrt(np.mean((final[inner] - true_model()[inner]) ** 2))
    print(f"\n[typed two-step] model error {e0:.4f} -> {e1:.4f} km/s")
    assert e1 < e0


def test_programs_that_refuse_typed_data_say_why(built, typed_case, tmp_path):
    sv, data = typed_case
    d = write_inputs(tmp_path / "joint", para_text(iso=False), data)
    out = run("DAzimSurfTomo_amd", d, ok=False)
    assert "joint mode" in out and "Rayleigh phase velocities only" in out and "Program finishes successfully" not in out
    d = write_inputs(tmp_path / "mc", para_text(), data)
    out = run("SurfDepthMC_amd", d, ok=False)
    assert "SurfDepthMC_amd" in out and "Monte-Carlo forward model is the" in out
    # a data type whose para.in block is missing: the message names the type and the line
    d = write_inputs(tmp_path / "missing", para_text(segments=T.SEGMENTS[:3]), data)
    out = run("DAzimSurfTomo_amd", d, ok=False)
    assert "Love group" in out and "kmaxLg" in out and "Program finishes successfully" not in out
    # 61 virtual periods: the column solve's limit
    many = [T.RC + (np.arange(5.0, 36.0),), T.RG + (np.arange(5.0, 35.0),)]
    d = write_inputs(tmp_path / "k61", para_text(segments=many), data)
    out = run("SurfDepthFromMaps_amd", d, ok=False)
    assert "at most 60" in out and "61" in out
