"""Inputs shared by tests/test_rays_step_forms_gpu.py and tools/rays_step_bits.py: three small ray batches that take the ray kernel's
stepping loop through its forms.

  base     the 17 x 15 x 4-knot, 3-period batch of tests/test_rays_gpu.py (build_case(..., 9, 6, 3)): steps with one, two and three
           sub-segments; rays that run up to 60 coarse cells from their source (far from its refined box) and end inside it
  edge     the same grid with every station in an edge cell of the node grid, 0.01 to 0.03 degrees inside the boundary: rays that run along the
           boundary are clipped to it (which resets the carried start-point term), and their velocities are taken in the last row and
           column of the grid (the general vel_at)
  refined  the same grid with every receiver within 0.35 degrees (seven of the eight coarse cells) of its source: whole rays inside
           the refined box

Dispersion inputs come from the CPU oracle, as in test_G_matches_oracle."""
import numpy as np

from tests import synth
from tests.test_disp_gpu import model
from tests.test_rays_gpu import build_case

NX, NY, KMAX, MINTHK = 17, 15, 3, 2.0
DEPZ = np.array([0.0, 10.0, 35.0, 60.0], np.float32)
T = np.array([8.0, 14.0, 22.0])
GOXD, GOZD, DV = 30.0, 100.0, 0.25
NAMES = ("base", "edge", "refined")


def _tables(lat, lon, pairs_of, nrc):
    """build_case's arrays for stations (lat, lon): source s of period k gets the receivers pairs_of(k, s)"""
    sx, sz = synth.radians(lat, lon)
    nsta = len(sx)
    scxf = np.zeros((KMAX, nsta), np.float32); sczf = scxf.copy()
    rcxf = np.zeros((KMAX, nsta, nrc), np.float32); rczf = rcxf.copy()
    nrc1 = np.zeros((KMAX, nsta), np.int32); nsrc1 = np.zeros(KMAX, np.int32); periods = np.zeros((KMAX, nsta), np.int32)
    for k in range(KMAX):
        nsrc1[k] = nsta
        for s in range(nsta):
            scxf[k, s] = sx[s]; sczf[k, s] = sz[s]; periods[k, s] = k + 1
            rx, rz = pairs_of(k, s, sx, sz)
            nrc1[k, s] = len(rx); rcxf[k, s, :len(rx)] = rx; rczf[k, s, :len(rx)] = rz
    return scxf, sczf, rcxf, rczf, nrc1, nsrc1, periods


def case(name):
    """(vel, scxf, sczf, rcxf, rczf, nrc1, nsrc1, periods) in build_case's layout"""
    if name == "base":
        return build_case(NX, NY, DEPZ, KMAX, 9, 6, 3)
    vel = model(NX, NY, DEPZ, 3)
    lat_hi, lat_lo = GOXD, GOXD - (NX - 3) * DV          # the node grid's extent, degrees
    lon_lo, lon_hi = GOZD, GOZD + (NY - 3) * DV
    if name == "edge":
        e, c = 0.01, 0.03   # (corner stations sit deeper in their cell: a source 0.01 degrees from a corner holds its rays at that corner
        #                      until the step limit, in the reference as here)
        lat = np.array([lat_hi - c, lat_hi - e, lat_hi - c, lat_lo + c, lat_lo + e, lat_lo + c, 29.1, 27.9, 28.7, 28.2], np.float32)
        lon = np.array([lon_lo + c, 101.4, lon_hi - c, lon_lo + c, 101.7, lon_hi - c, lon_lo + e, lon_lo + e, lon_hi - e, lon_hi - e], np.float32)

        def others(k, s, sx, sz):
            idx = [(s + 1 + k + i) % len(sx) for i in range(5)]
            idx = [i for i in idx if i != s]
            return sx[idx], sz[idx]
        return (vel,) + _tables(lat, lon, others, 5)
    if name == "refined":
        lat, lon = synth.stations(NX, NY, GOXD, GOZD, DV, DV, 6, seed=11, shrink=0.5)
        rng = np.random.default_rng(12)
        off = (rng.random((KMAX, 6, 4, 2)) * 0.6 - 0.3) + np.where(rng.random((KMAX, 6, 4, 2)) < 0.5, -0.05, 0.05)   # 0.05 .. 0.35 degrees

        def near(k, s, sx, sz):
            rx, rz = synth.radians(lat[s] + off[k, s, :, 0].astype(np.float32), lon[s] + off[k, s, :, 1].astype(np.float32))
            return rx, rz
        return (vel,) + _tables(lat, lon, near, 4)
    raise KeyError(name)


def sub_segments(path):
    """sub-segments of every step of a ray path [nrp][2] (receiver first, source last; the last point closes the path and is no
    step): 1 + the B-spline cell boundaries the step crosses in colatitude and in longitude"""
    gox, goz = synth.radians([GOXD], [GOZD])
    dv = DV * np.pi / 180.0
    p = np.asarray(path, np.float64)[:-1]
    ix, iz = np.floor((p[:, 0] - float(gox[0])) / dv), np.floor((p[:, 1] - float(goz[0])) / dv)
    return 1 + (np.diff(ix) != 0).astype(int) + (np.diff(iz) != 0).astype(int)
