"""Grids with unequal spacings and at other latitudes, shared by tests/golden/make_ref_geometries_golden.py,
tests/test_ref_geometries_cpu.py and tests/test_forward_geometries_gpu.py (plain module, no test in it).

A geometry is (goxd, gozd, dvxd, dvzd): latitude of the top vertex row and longitude of the left vertex column in degrees, and the
vertex spacings in latitude (x) and longitude (z).  Every other forward-path test passes one value for both spacings and sits at
26.5 .. 30 N, where an exchange of dnx and dnz changes no bit and the sine tables hold essentially one value.
"""
import numpy as np

from tests import synth

NX, NY = 12, 15                      # inversion grid of every case here: 10 x 13 vertices, 46 x 61 propagation nodes
NSRC = 6
SEED = 7                             # maps: synth.phase_velocity_maps(.., seed=SEED) / default_rng(SEED).uniform; stations: SEED + 1

# name -> (goxd, gozd, dvxd, dvzd)          node steps x / z in km
GEOMETRIES = {
    "wide_lon": (30.0, 100.0, 0.25, 0.4),   # 5.6 / 7.7-7.9   dz > dx
    "wide_lat": (30.0, 100.0, 0.5, 0.2),    # 11.1 / 3.9-4.0  dx > dz
    "north66": (66.0, 20.0, 0.2, 0.5),      # 4.4 / 4.5-4.8   small sine, steep change per row
    "south": (-30.0, 140.0, 0.3, 0.25),     # 6.7 / 4.8-4.7   colatitude > 90 deg, sine falling down the grid
    "equator": (2.0, -75.0, 0.4, 0.3),      # 8.9 / 6.7       crosses latitude 0, negative longitudes
    "fine72": (72.0, 10.0, 0.1, 0.15),      # 2.2 / 1.03-1.08 z step below 2 km: the short division's guard is off
}
NAMES = tuple(GEOMETRIES)


def tag(name, rough):
    """prefix of a case's arrays in tests/golden/ref_geometries.npz"""
    return f"{name}_{'rough' if rough else 'smooth'}"


def stations_inset(nx, ny, geo, n, seed, inset=0.6):
    """n stations (lat, lon in degrees, fp32) set in from every edge of the vertex box by `inset` cells of that axis"""
    goxd, gozd, dvxd, dvzd = geo
    rng = np.random.default_rng(seed)
    u, w = rng.random(n), rng.random(n)
    lat = (goxd - dvxd * (inset + u * ((nx - 3) - 2 * inset))).astype(np.float32)
    lon = (gozd + dvzd * (inset + w * ((ny - 3) - 2 * inset))).astype(np.float32)
    return lat, lon


def inset_callback(nx, ny, goxd, gozd, dvxd, dvzd, n, seed=1, shrink=None):
    """stations_inset with the signature of synth.stations (`shrink`, a distance in degrees, has no meaning here)"""
    return stations_inset(nx, ny, (goxd, gozd, dvxd, dvzd), n, seed)


def rough_map(shape, seed):
    """every inversion cell drawn independently from 2.0 .. 4.8 km/s, fp32-rounded (test_fmm_gpu._run_case(rough=True))"""
    return np.random.default_rng(seed).uniform(2.0, 4.8, shape).astype(np.float32).astype(np.float64)


def field_inputs(geo, rough, kmax=1, nx=NX, ny=NY, nsrc=NSRC, seed=SEED):
    """what test_fmm_gpu._run_case(nx, ny, kmax, nsrc, seed, *geo, stations=inset_callback, rough=rough) marches on:
    pv[kmax][nx*ny] and the sources' colatitudes / longitudes in radians (fp32).  Period 0 does not depend on kmax."""
    pv = synth.phase_velocity_maps(nx, ny, kmax, seed)
    if rough:
        pv = rough_map(pv.shape, seed)
    lat, lon = stations_inset(nx, ny, geo, nsrc, seed + 1)
    sx, sz = synth.radians(lat, lon)
    return pv, sx, sz


def extreme_velocity_map(kmax=2, nx=NX, ny=NY, seed=SEED):
    """the smooth maps with a 4 x 4 block of cells at 0.13 km/s and another at 15.9 km/s, just inside the range (0.125 .. 16 km/s)
    in which the eikonal kernel may use its short exact division; single cells elsewhere too"""
    pv = synth.phase_velocity_maps(nx, ny, kmax, seed).reshape(kmax, ny, nx)
    lo, hi = np.float64(np.float32(0.13)), np.float64(np.float32(15.9))
    pv[:, 2:6, 1:5] = lo
    pv[:, 8:12, 6:10] = hi
    pv[:, 12, 2] = hi
    pv[:, 4, 9] = lo
    return pv.reshape(kmax, ny * nx).copy()


def corner_and_node_sources(nx, ny, geo):
    """four sources exactly on the corner vertices and one exactly on a node (lat, lon in degrees): the clipped refined boxes"""
    goxd, gozd, dvxd, dvzd = geo
    lat = [goxd, goxd, goxd - (nx - 3) * dvxd, goxd - (nx - 3) * dvxd, goxd - 5 * dvxd]
    lon = [gozd, gozd + (ny - 3) * dvzd, gozd, gozd + (ny - 3) * dvzd, gozd + 7 * dvzd]
    return np.asarray(lat, np.float32), np.asarray(lon, np.float32)


# ---- rays ---------------------------------------------------------------------------------------------------------------------
RAY_DEPZ = np.array([0.0, 10.0, 35.0, 60.0], np.float32)
RAY_T = np.array([6.0, 14.0])
RAY_MINTHK = 2.0
DENSE_DEPZ = np.array([0.0, 12.0, 40.0], np.float32)
DENSE_T = np.array([8.0, 20.0])
DENSE_NAMES = ("wide_lon", "north66")


def ray_case(geo, depz=RAY_DEPZ, kmax=2, nsta=6, nrc=4, seed=SEED, nx=NX, ny=NY):
    """tests/test_rays_gpu.build_case's tuple (vel, scxf, sczf, rcxf, rczf, nrc1, nsrc1, periods) on a geometry, inset stations"""
    from tests.test_rays_gpu import build_case
    goxd, gozd, dvxd, dvzd = geo
    return build_case(nx, ny, depz, kmax, nsta, nrc, seed, goxd=goxd, gozd=gozd, dv=dvxd, dvz=dvzd, stations=inset_callback)


def dense_case(geo):
    """the 3-knot, 2-period batch whose dense copies GVs (GGc, GGs) the golden file records (6 stations, 3 receivers each)"""
    return ray_case(geo, depz=DENSE_DEPZ, kmax=2, nsta=6, nrc=3, seed=5)


# ---- the guard of the short exact division ------------------------------------------------------------------------------------
EARTH = np.float32(6371.0)
FAST_STEP_MIN = 2.0                  # km, fmm.hip


def node_steps(g):
    """the node steps in km as the host forms them for its guard: EARTH * g.dnx, and EARTH * sinf(gox + i*dnx) * g.dnz for every
    node row i (fp32 throughout; numpy's sine may differ from libm's in the last bit, which no case here comes near)"""
    f = np.float32
    sx = EARTH * f(g.dnx)
    colat = f(g.gox) + np.arange(g.nnx, dtype=np.float32) * f(g.dnx)
    sz = (EARTH * np.sin(colat)).astype(np.float32) * f(g.dnz)
    return float(abs(sx)), np.abs(sz).astype(np.float64)


def guard_edge_geometries():
    """name -> (geometry, fmm.fast_math expected, which premise holds); the premises are asserted by the test from node_steps().
    66 N, dvxd = 0.2 (x step 4.45 km): the z step is EARTH * sin(24.0 .. 25.8 deg) * dvzd/5, 9.045 .. 9.679 km per degree of dvzd."""
    return {
        "z_straddles_2km": ((66.0, 20.0, 0.2, 0.214), 0, "straddle"),      # 1.94 .. 2.07 km: top rows below 2 km, bottom rows above
        "z_just_above_2km": ((66.0, 20.0, 0.2, 0.222), 1, "just_above"),   # 2.01 .. 2.15 km: the smallest step in (2.0, 2.1]
        "x_alone_below_2km": ((10.0, 120.0, 0.08, 0.25), 0, "x_below"),    # x 1.78 km, z 5.5 km
    }
