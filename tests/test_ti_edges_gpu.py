"""-m gpu: dazim_ti_kernels (dazimsurftomo_amd/csrc/ti.hip) where its saturation branches switch and at the shapes where its lane,
block and layer limits lie -- the inputs of tests/ti_cases.py, which tests/test_ti_cases_cpu.py shows to take every guarded
exponential of tregn96 that an Earth column reaches (tests/test_ti_gpu.py's inputs take none).

Lsen is compared with the oracle (oracle/tregn.c, same phase velocities) and with the compiled reference's recorded output
(tests/golden/ti_stress.npz) by the three measures of tests/ti_cases.py: a. per lane to 1e-6 of the lane's maximum, b. per entry
down to 1e-30 to 4 x R_CPU, c. nothing above 1e-29 where the reference has less than 1e-30 or an exact zero; all finite.
Every figure is printed before it is asserted (pytest -s)."""
import os

import numpy as np
import pytest

from tests import ti_cases as K

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ti_stress.npz")
RUNS = K.stress_runs()


@pytest.fixture(scope="module")
def want(orc):
    """{key: (pv, lsen)} of the oracle on the six stress runs, computed once and left alone"""
    out = {}
    for key, name, minthk in RUNS:
        pv, ls = orc.depthkernel_ti(K.stress(name), K.DEPZ, K.T, minthk)
        pv.setflags(write=False); ls.setflags(write=False)
        out[key] = (pv, ls)
    return out


@pytest.fixture(scope="module")
def got(ctx, want):
    """{key: lsen} of the device on the six stress runs with the oracle's phase velocities"""
    out = {}
    for key, name, minthk in RUNS:
        out[key] = ctx.ti_kernels(K.stress(name), K.DEPZ, K.T, minthk, want[key][0])
        out[key].setflags(write=False)
    return out


def check_measures(what, lsen, ref, lane_tol=K.LANE_TOL, entry_tol=K.ENTRY_TOL_GPU):
    assert lsen.shape == ref.shape and lsen.dtype == np.float32, what
    assert np.isfinite(lsen).all(), what
    lane = K.lane_excess(lsen, ref)
    rel, at = K.entry_excess(lsen, ref)
    small = K.small_ceiling(lsen, ref)
    print(f"{what}: per lane {lane:.3g} (<= {lane_tol:g}); per entry {rel:.3g} at (layer, period, column) {at} (<= {entry_tol}); "
          f"largest |got| where |want| < {K.ENTRY_FLOOR:g}: {small:.3g} (< {K.ZERO_CEIL:g})")
    assert lane <= lane_tol, (what, "measure a", lane)
    if entry_tol is not None:
        assert rel <= entry_tol, (what, "measure b", rel, at, float(lsen[at]), float(ref[at]))
        assert small < K.ZERO_CEIL, (what, "measure c", small)


@pytest.mark.parametrize("key", [r[0] for r in RUNS])
def test_stress_models_vs_oracle_and_reference(got, want, key):
    gold = np.load(GOLD)
    assert np.array_equal(want[key][0], gold[f"{key}_pv"])        # the golden was recorded at the phase velocities used here
    check_measures(f"{key} vs oracle", got[key], want[key][1])
    check_measures(f"{key} vs reference", got[key], gold[f"{key}_lsen"])


@pytest.mark.parametrize("key", [r[0] for r in RUNS])
def test_stress_models_with_the_devices_own_phase_velocities(ctx, want, key):
    """pvRc of the device may differ from the oracle's by an fp32 ulp (tests/test_disp_gpu.py): the 2e-5 bar of
    tests/test_ti_gpu.py, per lane"""
    _, name, minthk = next(r for r in RUNS if r[0] == key)
    vel = K.stress(name)
    pv, _, nf = ctx.depthkernel(vel, K.DEPZ, K.T, minthk, kernels=False)
    assert nf == 0
    print(f"{key}: max |pv - pv_oracle| {np.abs(pv - want[key][0]).max():.3g}")
    lsen = ctx.ti_kernels(vel, K.DEPZ, K.T, minthk, pv)
    check_measures(f"{key}, device pv, vs oracle", lsen, want[key][1], lane_tol=2e-5, entry_tol=None)


# ---- lane and block tails ----
@pytest.mark.parametrize("case", ["lanes_60", "columns_129", "two_knots"])
def test_lane_and_block_tails(ctx, orc, case):
    c = getattr(K, case)()
    pv, ls = orc.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
    assert (pv > 0).all()
    lsen = ctx.ti_kernels(c["vel"], c["depz"], c["t"], c["minthk"], pv)
    check_measures(case, lsen, ls)


def test_61_periods_are_refused(ctx, got):
    import dazimsurftomo_amd as dz
    c = K.lanes_60()
    t = np.linspace(4.0, 34.0, 61)
    with pytest.raises(dz.DazimError):
        ctx.ti_kernels(c["vel"], c["depz"], t, c["minthk"], np.full((61, 1), 3.0))
    again(ctx, got)


def again(ctx, got):
    """the context computes stress model A at minthk 1 again, bit for bit as before"""
    pv = np.load(GOLD)["A_1_pv"]
    assert np.array_equal(ctx.ti_kernels(K.stress("A"), K.DEPZ, K.T, 1.0, pv), got["A_1"])


# ---- layer limit and errors ----
def test_200_layers_fit_201_do_not(ctx, orc, got):
    import dazimsurftomo_amd as dz
    c = K.layer_limit(200)
    pv, ls = orc.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
    assert (pv > 0).all()
    lsen = ctx.ti_kernels(c["vel"], c["depz"], c["t"], c["minthk"], pv)
    check_measures("mmax = 200", lsen, ls)
    c = K.layer_limit(201)
    with pytest.raises(dz.DazimError, match="201 layers"):
        ctx.ti_kernels(c["vel"], c["depz"], c["t"], c["minthk"], np.full((3, 2), 3.5))
    again(ctx, got)


def test_fluid_layer_is_refused(ctx, orc, got):
    import dazimsurftomo_amd as dz
    c = K.fluid_column()
    with pytest.raises(RuntimeError, match="rc=3"):
        orc.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
    with pytest.raises(dz.DazimError, match="fluid layer"):
        ctx.ti_kernels(c["vel"], c["depz"], c["t"], c["minthk"], np.full((2, 1), 3.0))
    again(ctx, got)


# ---- rootless lanes ----
def test_scattered_rootless_lanes(ctx, want, got):
    """pv = 0, negative or NaN: no kernel for that lane (all zeros), every other lane untouched"""
    pv = want["B_3"][0].copy()
    dead = [(0, 0, 0.0), (0, 20, -3.1), (2, 7, np.nan), (3, 8, 0.0), (5, 13, -0.0), (7, 20, np.nan), (7, 0, -1e-300)]
    for k, col, v in dead:
        pv[k, col] = v
    lsen = ctx.ti_kernels(K.stress("B"), K.DEPZ, K.T, 3.0, pv)
    mask = np.zeros(lsen.shape[1:], bool)
    for k, col, _ in dead:
        mask[k, col] = True
    assert (lsen[:, mask] == 0).all() and not np.signbit(lsen[:, mask]).any()
    assert np.array_equal(lsen[:, ~mask], got["B_3"][:, ~mask])


def test_a_whole_wavefront_without_root(ctx, orc):
    """64 columns: period row 1 is exactly the lanes of the second wavefront, which leaves at once"""
    c = K.wavefront_row()
    pv, ls = orc.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
    full = ctx.ti_kernels(c["vel"], c["depz"], c["t"], c["minthk"], pv)
    check_measures("64 columns", full, ls)
    pv0 = pv.copy()
    pv0[1, :] = 0.0
    lsen = ctx.ti_kernels(c["vel"], c["depz"], c["t"], c["minthk"], pv0)
    assert (lsen[:, 1, :] == 0).all()
    assert np.array_equal(lsen[:, [0, 2], :], full[:, [0, 2], :])


# ---- state ----
def test_scratch_reuse_across_shapes(ctx, orc, want, got):
    """168 lanes, then 60 lanes on a 1 x 1 model, then 168 again on one context: the named scratch buffers are reused with another
    [layer][value][lane] stride"""
    vel, pv = K.stress("A"), want["A_3"][0]
    first = ctx.ti_kernels(vel, K.DEPZ, K.T, 3.0, pv)
    c = K.lanes_60()
    pv1, _ = orc.depthkernel_ti(c["vel"], c["depz"], c["t"], c["minthk"])
    small1 = ctx.ti_kernels(c["vel"], c["depz"], c["t"], c["minthk"], pv1)
    second = ctx.ti_kernels(vel, K.DEPZ, K.T, 3.0, pv)
    small2 = ctx.ti_kernels(c["vel"], c["depz"], c["t"], c["minthk"], pv1)
    assert np.array_equal(first, got["A_3"]) and np.array_equal(second, first) and np.array_equal(small1, small2)


def test_device_tensors_give_the_bits_of_host_arrays(ctx, want, got):
    import torch
    out = ctx.ti_kernels(torch.from_numpy(K.stress("B")).cuda(), K.DEPZ, K.T, 0.5, torch.from_numpy(want["B_0.5"][0].copy()).cuda())
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), got["B_0.5"])


def test_raised_priority_launch_gives_the_same_bits(want, got):
    """behind an asynchronous dispersion call (its perturbed copies pending on the auxiliary stream) ti_kernel raises its
    wavefronts' issue priority: the same bits as the plain launch"""
    import torch
    import dazimsurftomo_amd as dz
    d_vel = torch.from_numpy(K.stress("A")).cuda()
    d_pv = torch.from_numpy(want["A_1"][0].copy()).cuda()
    c = dz.Context(0)
    try:
        c.set_option("disp.async", 2)
        tables = c.depthkernel(d_vel, K.DEPZ, K.T, 1.0)    # (held until the copies that fill them are joined)
        assert c.kernel_seconds("disp.async") == 1 and c.stat("aux.pending") == 1
        out = c.ti_kernels(d_vel, K.DEPZ, K.T, 1.0, d_pv)
        c.sync()
        assert np.array_equal(out.cpu().numpy(), got["A_1"])
        del tables
    finally:
        c.close()
