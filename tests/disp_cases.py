"""Inputs shared by tests/test_disp_cases_cpu.py, tests/test_disp_edges_gpu.py and tests/golden/make_disp_stress_golden.py: the
stress columns of tests/ti_cases.py put through the ISOTROPIC dispersion path (oracle/disp.c, dazimsurftomo_amd/csrc/disp.hip)
where surfdisp96's guards and its root search switch -- the branches that the inputs of tests/test_disp_gpu.py never take -- and
the first periods at which disp_bracket_kernel's 64-point blocks hand over (no GPU import).

A case is dict(vel[nz][ny][nx] fp32, depz, t, minthk, kernels).  Branch names are those of oracle.pyoracle.DISP_CENSUS.

  stress runs    models A and B at minthk 0.5, 1, 3 with depth kernels: 21 columns x 49 variants x 8 periods.  Thick deep layers
                 at short periods: p >= 16, q >= 16 (exp(-2p), exp(-2q) taken as 0) and p + q >= 60 (a0 = 0) on 14-35 % of the
                 layer visits; B at minthk 1 and 3 runs faster than its sediment's Vp at 40 s (oscillatory P)
  short          A and B at 0.2 .. 1 s: three quarters of the visits saturated in both parts
  orders         B with the periods decreasing (every search but the first starts downwards) and shuffled (Neville's c3 leaves
                 the bracket; one interpolation is abandoned at the denominator guard)
  long           periods 1e5 s and 1e6 s appended: omega < 1e-4 is clamped, and both periods fail in every column, the walk
                 ending at betmx + dc
  first fails    three narrow columns whose FIRST period (1e5 s) has no root: every period of the column is 0; the walk of
                 column 0 meets betmx + dc at grid point 251 = 3 x 64 + 59, inside a block of disp_bracket_kernel
  long walk      B at minthk 3 with 80 s first: every column's bracket lies beyond the 8 x 64 = 512 points disp_bracket_kernel
                 evaluates (the kernel reports "not found", the search goes step by step)
  B_2            B at minthk 2: nsub = 3, 2 nsub = 6, the reciprocal + correction form of the sub-layer interpolation (division
                 class 2, with disp.rden = 0 class 0); the stress minthk values give powers of two (class 1)
  planted        one column, a first period chosen so that the bracket's lower end is grid point 62, 63, 64, 127, 128, 510, 511
                 or 512.  The sign changes at the point after it: 62 -> lane 63 of the kernel's block 0; 63 and 127 -> lane 0 of
                 blocks 1 and 2, where the sign and the c of the block before are what the kernel carried over; 64 and 128 ->
                 lane 1; 510 -> point 511, the last one the kernel evaluates; 511 and 512 -> not found
"""
import os

import numpy as np

from tests.ti_cases import DEPZ, T, stress, stress_runs      # (stress_runs: models A, B x MINTHKS)

T_SHORT = np.array([0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 1.0])
T_LONG = np.array([5.0, 8.0, 15.0, 40.0, 1.0e5, 1.0e6])
T_80_FIRST = np.concatenate([[80.0], T])
T_80_SHORT = np.array([80.0, 1.0, 5.0, 40.0])
SHUFFLE = np.array([2, 5, 3, 7, 0, 4, 1, 6])           # np.random.default_rng(6).permutation(8), written out
FF_POINTS = 512                                          # grid points disp_bracket_kernel evaluates (FF_BLOCKS x 64)

# the branches the new inputs must take (each on the run named in REACHED_BY), and the ones nothing here takes
SATURATION = ("p_sat", "s_sat", "a0_zero")
MUST_REACH = SATURATION + ("p_osc", "omega_clamp", "getsol_down", "nev_c3_out", "nev_denom", "exit_window", "first_over_512")
REACHED_BY = {"p_sat": "A_0.5", "s_sat": "A_0.5", "a0_zero": "A_0.5", "p_osc": "B_3", "omega_clamp": "B_1_long",
              "getsol_down": "B_1_decreasing", "nev_c3_out": "B_1_shuffled", "nev_denom": "B_1_shuffled",
              "exit_window": "A_1_long", "first_over_512": "B_3_80first"}
NOT_REACHED = ("p_equal", "s_equal", "t1_tiny", "nev_m_cap", "nev_nctrl", "getsol_turn", "exit_below_cm", "exit_root_above")


def _case(vel, depz, t, minthk, kernels=True):
    return dict(vel=np.ascontiguousarray(vel, np.float32), depz=np.asarray(depz, np.float32), t=np.asarray(t, np.float64),
                minthk=float(minthk), kernels=kernels)


def narrow_columns():
    """4-knot columns between 3.0 and 3.6 km/s: the search window [cc, betmx + dc] is 1.0 to 1.3 km/s wide, and at 1e5 s (omega
    clamped) the secular function has no sign change in it.  Walks of 251, 202 and 235 steps to betmx + dc."""
    vel = np.array([[3.0, 3.2, 3.4, 3.6], [3.2, 3.3, 3.4, 3.5], [3.1, 3.3, 3.3, 3.6]], np.float32).T.reshape(4, 1, 3)
    return vel, np.array([0.0, 10.0, 20.0, 40.0], np.float32)


def planted_column():
    """column 0 of stress model B: a 1.16 km/s sediment, so the search starts below 1 km/s, and the fundamental mode climbs from
    1.65 km/s at 0.95 s to 3.9 km/s at 68 s, 512 steps of dc above the start"""
    return np.ascontiguousarray(stress("B")[:, :1, :1])


# first period -> grid point of the bracket's lower end (= dc steps walked, census first_steps_max), column planted_column() at
# minthk 1.  Found by bisection on the CPU (the root moves continuously with T); each period is the middle of the interval of T
# that gives the step count, rounded: 0.9407-0.9541, 0.9541-0.9670, 0.9670-0.9794, 1.4257-1.4309, 1.4309-1.4361, 66.51-67.23,
# 67.23-67.97, 67.97-68.73 s.
PLANTED = ((0.9474, 62), (0.9605, 63), (0.9732, 64), (1.4283, 127), (1.4335, 128), (66.87, 510), (67.6, 511), (68.35, 512))
FOUND_BY_BRACKET_KERNEL = (62, 63, 64, 127, 128, 510)   # a sign change among the FF_POINTS grid points 0 .. 511
PLANTED_TAIL = (20.0, 5.0, 1.5)      # the periods searched after the planted one


def cases():
    """{name: case}, in a fixed order; every case has depth kernels (49 or 25 variants per column) unless it says otherwise"""
    out = {}
    for key, name, minthk in stress_runs():
        out[key] = _case(stress(name), DEPZ, T, minthk)
    for name in ("A", "B"):
        out[f"{name}_1_short"] = _case(stress(name), DEPZ, T_SHORT, 1.0)
    out["B_1_decreasing"] = _case(stress("B"), DEPZ, T[::-1], 1.0)
    out["B_1_shuffled"] = _case(stress("B"), DEPZ, T[SHUFFLE], 1.0)
    for name in ("A", "B"):
        out[f"{name}_1_long"] = _case(stress(name), DEPZ, T_LONG, 1.0)
    vel, depz = narrow_columns()
    out["first_fails"] = _case(vel, depz, [1.0e5, 10.0, 20.0], 2.0)
    out["A_1_80first"] = _case(stress("A"), DEPZ, T_80_FIRST, 1.0)      # 8 (column, period) pairs fail in mid-curve
    out["B_3_80first"] = _case(stress("B"), DEPZ, T_80_SHORT, 3.0)
    out["B_2"] = _case(stress("B"), DEPZ, T, 2.0)
    for t1, steps in PLANTED:
        out[f"planted_{steps}"] = _case(planted_column(), DEPZ, (t1,) + PLANTED_TAIL, 1.0)
    return out


STRESS_KEYS = tuple(k for k, _, _ in stress_runs())
GOLDEN_KEYS = STRESS_KEYS + ("A_1_short", "B_1_short")      # what tests/golden/disp_stress.npz holds
EXP_KEYS = GOLDEN_KEYS                                       # both exponential forms are compared on these
FFWD_KEYS = tuple(f"planted_{s}" for _, s in PLANTED) + ("B_3_80first", "A_1_80first", "first_fails")


def attempts():
    """honest attempts at the branches of NOT_REACHED, still Earth columns:
      0  a 360 km layer at 0.2 s and 0.5 s (the compound vector shrinks by exp(-p-q) per layer: t1 < 1e-40 needs it to underflow
         inside one layer, but a0 is cut to 0 at 60 and the vector is rescaled after every layer)
      1  model A, periods shuffled so that the curve is searched downwards to the lower bound (c2 <= clow, c1 < cm)
      2  a low-velocity half-space under a fast lid (a root above betmx, were the window not closed at betmx + dc first)
      3  a phase velocity equal to a layer's Vp or Vs to the last bit (wvno == xka, xkb): 60 periods across a two-layer model"""
    depz = np.array([0.0, 3.0, 15.0, 40.0, 400.0], np.float32)
    vel = np.array([2.6, 3.3, 3.7, 4.4, 4.8], np.float32).reshape(5, 1, 1)
    out = [_case(vel, depz, [0.2, 0.5], 0.5)]
    out.append(_case(stress("A"), DEPZ, T[[1, 2, 0, 7, 4, 5, 3, 6]], 1.0))
    depz = np.array([0.0, 10.0, 20.0, 40.0], np.float32)
    out.append(_case(np.array([4.6, 4.4, 3.0, 2.6], np.float32).reshape(4, 1, 1), depz, [5.0, 10.0, 20.0, 40.0, 60.0], 2.0, kernels=False))
    vel = np.array([3.0, 4.5], np.float32).reshape(2, 1, 1)
    out.append(_case(vel, np.array([0.0, 20.0], np.float32), np.linspace(2.0, 60.0, 60), 0.5, kernels=False))
    return out


def old_inputs():
    """every oracle run tests/test_disp_gpu.py makes (its failing column included, and the column it used before that, which never
    failed), and the failure column of tests/test_disp_shared_layers_gpu.py: the negative control"""
    from tests.test_disp_gpu import ROUGH_DEPZ, ROUGH_T, model, no_root_column
    runs = []
    depz = np.array([0.0, 10.0, 35.0, 60.0], np.float32)
    runs.append(_case(model(6, 5, depz, 1), depz, np.arange(5, 41, dtype=np.float64), 2.0))
    depz = np.arange(12, dtype=np.float32) * 5.0
    runs.append(_case(model(4, 3, depz, 2), depz, np.arange(5, 37, 2, dtype=np.float64), 3.0))
    runs.append(_case(model(6, 5, depz, 12), depz, np.arange(5, 37, 2, dtype=np.float64), 3.0))
    depz = np.array([0, 3, 6, 9, 12, 16, 20, 25, 30, 35, 40, 50, 60, 70, 80, 100, 120, 150], np.float32)
    runs.append(_case(model(3, 2, depz, 3), depz, np.arange(5, 41, dtype=np.float64), 4.0))
    depz = np.array([0.0, 5.0, 10.0, 20.0, 35.0, 60.0], np.float32)
    vel = np.zeros((6, 2, 3), np.float32)
    vel[:] = np.array([3.4, 3.6, 2.9, 3.2, 3.9, 4.4], np.float32)[:, None, None]
    vel[:, 1, :] *= np.float32(1.03)
    runs.append(_case(vel, depz, np.arange(4, 44, 2, dtype=np.float64), 3.0, kernels=False))
    depz = np.array([0.0, 10.0, 20.0, 40.0], np.float32)
    vel = np.zeros((4, 1, 2), np.float32)
    vel[:, 0, 0] = [3.0, 3.5, 3.9, 4.3]
    vel[:, 0, 1] = [4.6, 4.4, 3.0, 2.6]
    runs.append(_case(vel, depz, [5.0, 10.0, 20.0, 40.0, 60.0], 2.0, kernels=False))
    runs.append(_case(no_root_column(), ROUGH_DEPZ, ROUGH_T, 3.0))
    rng = np.random.default_rng(5)
    vel = rng.uniform(2.6, 4.7, (len(ROUGH_DEPZ), 20, 30)).astype(np.float32)
    vel[-1] = np.maximum(vel[-1], 4.2)
    runs.append(_case(vel, ROUGH_DEPZ, ROUGH_T, 3.0, kernels=False))
    return runs


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disp_stress.npz")
