"""Inputs shared by tests/test_ti_cases_cpu.py, tests/test_ti_edges_gpu.py and tests/golden/make_ti_stress_golden.py: layered
columns that take the TI depth-kernel path (oracle/tregn.c, dazimsurftomo_amd/csrc/ti.hip) through the guarded exponentials of
tregn96 -- the branches that the test4, test1 and random 5-knot inputs of tests/test_ti_gpu.py never take -- and the shapes at
which ti.hip's lane, block and layer limits switch (no GPU import).

  stress("A")  an 8-knot crustal column down to 200 km, 3 % lateral noise, 3 x 7 columns, periods 1 s to 40 s: thick deep layers at
               short periods saturate every scaled exponential
  stress("B")  the same knots with a 1.2 km/s sediment on top and a low-velocity zone at 14 to 30 km, 2 % noise: at minthk 1 and 3
               the 40 s wave runs faster than the top sublayer's Vp (imaginary nu_p)

each at MINTHKS (`nsub = int(minthk) + 1` sublayers per knot interval: the SMALL minthk gives the thick layers).  21 columns x 8
periods = 168 lanes: two full 64-lane wavefronts and a tail of 40.

The measures every comparison of Lsen uses (Lsen spans more than 30 decades over depth and period, so a bound relative to the
array's maximum sees the shallow long-period entries only):
  a. per (period, column) lane: max_j |got - want| <= LANE_TOL * max_j |want|
  b. per entry with |want| >= ENTRY_FLOOR: |got - want| <= bound * |want|
  c. per entry with |want| < ENTRY_FLOOR (the exact zeros included): |got| < ZERO_CEIL; everything finite
"""
import numpy as np

DEPZ = np.array([0, 2, 6, 14, 30, 60, 120, 200], np.float32)
T = np.array([1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 15.0, 40.0])
MINTHKS = (0.5, 1.0, 3.0)
V1D = {"A": [2.4, 3.0, 3.4, 3.7, 4.0, 4.4, 4.5, 4.7], "B": [1.2, 3.2, 3.6, 3.1, 3.0, 4.3, 4.5, 4.7]}
NOISE = {"A": 0.03, "B": 0.02}
SHAPE = (8, 3, 7)          # nz, ny, nx

LANE_TOL = 1e-6            # the project's TI bar (tests/test_ti_gpu.py), per lane here
ENTRY_FLOOR = 1e-30
ZERO_CEIL = 1e-29
# largest per-entry relative deviation of the oracle from the compiled reference over the six stress runs, all non-zero
# entries (1 down to 2e-36): 4.94e-7 (run A at minthk 1) as tests/test_ti_cases_cpu.py::test_oracle_against_reference measures
# it, rounded up
R_CPU = 5.0e-7
# device bound of measure b: 4 x the spread of two fp64 restatements (last-place libm results and the order of the compound
# products, carried through at most 22 exponent sums)
ENTRY_TOL_GPU = 4 * R_CPU

# the branches the stress runs must take (names of oracle.pyoracle.TI_CENSUS), and the ones no Earth column reached
SATURATION = ("fac0", "dfac0", "ffunc", "gfunc", "h1func", "h2func", "ext80", "flush")
MUST_REACH = SATURATION + ("imag_rsv", "imag_rp")
NOT_REACHED = ("down0", "t1_up", "t1_down", "tiny_nu")


def stress(name):
    """vel[8][3][7] fp32 of stress model A or B (one generator, A drawn first, B second)"""
    rng = np.random.default_rng(5)
    out = {}
    for k in ("A", "B"):
        out[k] = (np.array(V1D[k])[:, None, None] * (1 + NOISE[k] * rng.standard_normal(SHAPE))).astype(np.float32)
    return out[name]


def stress_runs():
    """(key, model name, minthk) of the six runs; key names the golden's arrays (`<key>_pv`, `<key>_lsen`)"""
    return [(f"{m}_{minthk:g}", m, minthk) for m in ("A", "B") for minthk in MINTHKS]


def thick_deep_layer():
    """one very thick deep layer at T = 1 s: the single attempt at the branches of NOT_REACHED (still an Earth column)"""
    depz = np.array([0.0, 3.0, 15.0, 40.0, 400.0], np.float32)
    vel = np.array([2.6, 3.3, 3.7, 4.4, 4.8], np.float32).reshape(5, 1, 1)
    return dict(vel=vel, depz=depz, t=np.array([1.0, 2.0]), minthk=0.5)


def old_inputs():
    """(vel, depz, t, minthk) of every oracle run tests/test_ti_gpu.py makes, and of its test1 model: the negative control"""
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gold, "test4_yunnan.npz"))
    vel = np.ascontiguousarray(g["vel"][:, 18:22, 6:14])
    t = np.arange(5, 41, dtype=np.float64)
    runs = [(vel, g["depz"], t, 2.0), (vel, g["depz"], t, 4.0)]
    a = np.load(os.path.join(gold, "test1_authors.npz"))
    runs.append((a["vel"], a["depz"], a["periods"], 2.0))
    rng = np.random.default_rng(3)
    depz = np.array([0.0, 4.0, 10.0, 20.0, 38.0], np.float32)
    v1d = np.array([3.0, 3.3, 3.6, 3.9, 4.3], np.float32)
    vel = (v1d[:, None, None] * (1 + 0.05 * rng.standard_normal((5, 4, 6)))).astype(np.float32)
    runs.append((vel, depz, np.array([5.0, 9.0, 14.0, 25.0]), 3.0))
    return runs


# ---- shapes at which ti.hip takes another path ----
def lanes_60():
    """kmax = 60 (the limit) on a 1 x 1 model: 60 lanes, less than one wavefront"""
    depz = np.array([0.0, 5.0, 15.0, 35.0], np.float32)
    vel = np.array([3.0, 3.4, 3.8, 4.4], np.float32).reshape(4, 1, 1)
    return dict(vel=vel, depz=depz, t=np.linspace(4.0, 33.5, 60), minthk=2.0)


def columns_129():
    """kmax = 1 with 129 columns: ti_model_kernel's 128-thread block tail and a one-lane wavefront tail"""
    rng = np.random.default_rng(21)
    depz = np.array([0.0, 5.0, 15.0, 35.0], np.float32)
    v1d = np.array([3.0, 3.4, 3.8, 4.4])
    vel = (v1d[:, None, None] * (1 + 0.03 * rng.standard_normal((4, 1, 129)))).astype(np.float32)
    return dict(vel=vel, depz=depz, t=np.array([10.0]), minthk=2.0)


def two_knots():
    """nz = 2: one interval and the half-space, nsub = 1"""
    vel = np.array([[[3.0, 3.2, 2.9]], [[4.2, 4.0, 4.3]]], np.float32)
    return dict(vel=vel, depz=np.array([0.0, 12.0], np.float32), t=np.array([3.0, 8.0, 20.0]), minthk=0.5)


def layer_limit(nknot):
    """nknot knots at 1 km spacing, minthk 0.5 (nsub = 1): mmax = nknot refined layers; 200 = NL is the last size that fits"""
    depz = np.arange(nknot, dtype=np.float32)
    rng = np.random.default_rng(31)
    v1d = 2.8 + 0.009 * depz
    vel = (v1d[:, None, None] * (1 + 0.01 * rng.standard_normal((nknot, 1, 2)))).astype(np.float32)
    return dict(vel=vel, depz=depz, t=np.array([6.0, 15.0, 40.0]), minthk=0.5)


def fluid_column():
    """Vs = 0.005 km/s at the two top knots (a sublayer takes its Vs between its two knots, never at one): TL <= 1e-4 TA, the fluid
    layer neither tregn.c nor ti.hip restates (oracle: 3)"""
    depz = np.array([0.0, 5.0, 15.0, 35.0], np.float32)
    vel = np.array([0.005, 0.005, 3.8, 4.4], np.float32).reshape(4, 1, 1)
    return dict(vel=vel, depz=depz, t=np.array([10.0, 20.0]), minthk=2.0)


def wavefront_row():
    """64 columns x 3 periods: one period row is one whole wavefront"""
    rng = np.random.default_rng(41)
    depz = np.array([0.0, 4.0, 10.0, 20.0, 38.0], np.float32)
    v1d = np.array([3.0, 3.3, 3.6, 3.9, 4.3])
    vel = (v1d[:, None, None] * (1 + 0.04 * rng.standard_normal((5, 8, 8)))).astype(np.float32)
    return dict(vel=vel, depz=depz, t=np.array([6.0, 12.0, 24.0]), minthk=3.0)


# ---- the three measures ----
def lane_excess(got, want):
    """measure a: max over lanes of (max_j |got - want|) / (max_j |want|), 0 where a lane's want is all zero and got equals it"""
    d = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=0)
    w = np.abs(want.astype(np.float64)).max(axis=0)
    if (d[w == 0] != 0).any():
        return np.inf
    return float((d[w > 0] / w[w > 0]).max()) if (w > 0).any() else 0.0


def entry_excess(got, want, floor=ENTRY_FLOOR):
    """measure b: (largest |got - want| / |want| over the non-zero entries with |want| >= floor, its index); floor 0: every non-zero
    entry"""
    g, w = got.astype(np.float64), want.astype(np.float64)
    m = (np.abs(w) >= floor) & (w != 0)
    if not m.any():
        return 0.0, None
    r = np.zeros_like(w)
    r[m] = np.abs(g - w)[m] / np.abs(w)[m]
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), tuple(int(x) for x in i)


def small_ceiling(got, want):
    """measure c: largest |got| over the entries with |want| < ENTRY_FLOOR (0.0 if there are none)"""
    m = np.abs(want.astype(np.float64)) < ENTRY_FLOOR
    return float(np.abs(got[m].astype(np.float64)).max()) if m.any() else 0.0
