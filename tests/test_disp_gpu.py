"""-m gpu: dispersion + depth kernels on the device (dazim_dispersion_kernels) against the oracle.

Tolerance, stated and justified: the root search is fp64 and the device's exp/sin/cos/sqrt differ
from glibc's in the last bit, so the converged root can differ by a few 1e-16 relative -- invisible
after the reference's own rounding cg(k)=sngl(c(k)) except when the root sits on an fp32 rounding
boundary or a convergence test (|c1-c2| <= 1e-6*c1, inv/surfdisp96.f:608) flips.  Hence:
  pvRc : |d| <= one fp32 ulp and bit-equal on >= 99.9 % of entries (measured: bit-equal everywhere on layered models);
  sen_*: |d| <= 2e-5 abs (one-ulp flip of c divided by 0.01*v) and relative L2 error <= 1e-6
  (see the constants below; columns of independent random knots have their own, measured, bars).
"""
import numpy as np
import pytest

from tests.bars import at_least, within

pytestmark = pytest.mark.gpu


def model(nx, ny, depz, seed):
    rng = np.random.default_rng(seed)
    nz = len(depz)
    base = 3.0 + 0.03 * np.asarray(depz)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    v = np.zeros((nz, ny, nx), np.float32)
    for k in range(nz):
        checker = np.where(((ii // 3) + (jj // 3) + k // 2) % 2 == 0, 1.0, -1.0)
        v[k] = np.clip(base[k] * (1 + 0.06 * checker) + 0.02 * rng.standard_normal((ny, nx)), 2.5, 4.8)
    return v


# the bars (DESIGN.md section 5 quotes the measured maxima they are twice of)
# Measured (MI355X, round 3): pvRc and sen_* are BIT-EQUAL to the oracle on every layered model of this file and of the examples
# (max |d| = 0, share 1.0); only columns whose knots are drawn independently at random differ (max 2.9e-6 km/s, 0.4 % of the
# entries: the root tolerance 1e-6 c decides).  Bars: one fp32 ulp of c on at most 0.1 % of the entries for models (SURVEY 8d's
# proposal), twice the measured figures for the rough random columns.
PV_ABS = 4.8e-7          # km/s: one ulp of an fp32 phase velocity in 4..8 km/s
PV_EQUAL_SHARE = 0.999   # share of bit-equal pvRc entries
PV_ABS_ROUGH, PV_EQUAL_SHARE_ROUGH = 6e-6, 0.9925
SEN_REL, SEN_ABS = 0.0, 2e-5   # one-ulp flip of c divided by 0.01 v
SEN_L2 = 1e-6


def compare(ctx, orc, vel, depz, t, minthk):
    pv, sen, nf = ctx.depthkernel(vel, depz, t, minthk)
    pvo, seno = orc.depthkernel(vel, depz, t, minthk)
    assert nf == int((pvo == 0).sum())
    d = np.abs(pv - pvo)
    share = (pv == pvo).mean()
    sd = [np.abs(a - b).max() for a, b in zip(sen, seno)]
    sl = [np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(sen, seno)]
    print(f"\n[disp parity] pv max |d| {d.max():.2e} bit-equal {share:.5f}; sen max |d| {max(sd):.2e} "
          f"(max |sen| {max(np.abs(b).max() for b in seno):.2e}) rel-L2 {max(sl):.2e}")
    within("pvRc max |d| km/s", d.max(), PV_ABS)
    at_least("pvRc bit-equal share", share, PV_EQUAL_SHARE)
    for a, b in zip(sen, seno):
        within("sen max |d|", np.abs(a - b).max(), SEN_REL * np.abs(b).max() + SEN_ABS)
        within("sen rel-L2", np.linalg.norm(a - b) / np.linalg.norm(b), SEN_L2)
    return pv, pvo


def test_depthkernel_test1_like(ctx, orc):
    """nz=4 knots at 0,10,35,60 km, sublayers=2 (rmax=10), 36 periods 5..40 s: the test1-3 setup"""
    depz = np.array([0.0, 10.0, 35.0, 60.0], np.float32)
    vel = model(6, 5, depz, 1)
    compare(ctx, orc, vel, depz, np.arange(5, 41, dtype=np.float64), 2.0)


def test_depthkernel_s256_like(ctx, orc):
    """nz=12 knots every 5 km, sublayers=3 (rmax=45), 16 periods 5..35 s: the S-256 column model"""
    depz = np.arange(12, dtype=np.float32) * 5.0
    vel = model(4, 3, depz, 2)
    compare(ctx, orc, vel, depz, np.arange(5, 37, 2, dtype=np.float64), 3.0)


def test_depthkernel_deep_model(ctx, orc):
    """test4-like: 18 knots to 150 km, sublayers=4 (rmax=69), 36 periods"""
    depz = np.array([0, 3, 6, 9, 12, 16, 20, 25, 30, 35, 40, 50, 60, 70, 80, 100, 120, 150], np.float32)
    vel = model(3, 2, depz, 3)
    compare(ctx, orc, vel, depz, np.arange(5, 41, dtype=np.float64), 4.0)


def test_phase_only_and_low_velocity_zone(ctx, orc):
    """kernels=False path (CalRayleighPhase) on a model with a strong low-velocity zone, which makes
    the bracket search walk in both directions (reversed dispersion, inv/surfdisp96.f:426-432)"""
    depz = np.array([0.0, 5.0, 10.0, 20.0, 35.0, 60.0], np.float32)
    vel = np.zeros((6, 2, 3), np.float32)
    vel[:] = np.array([3.4, 3.6, 2.9, 3.2, 3.9, 4.4], np.float32)[:, None, None]
    vel[:, 1, :] *= np.float32(1.03)
    t = np.arange(4, 44, 2, dtype=np.float64)
    pv, sen, nf = ctx.depthkernel(vel, depz, t, 3.0, kernels=False)
    pvo, _ = orc.depthkernel(vel, depz, t, 3.0, kernels=False)
    assert sen is None
    within("LVZ pvRc max |d| km/s", np.abs(pv - pvo).max(), PV_ABS)


def no_root_column():
    """vel[10][1][2] on ROUGH_DEPZ: a fast lid over slow channels, whose search leaves the window (c1 >= betmx + dc,
    inv/surfdisp96.f:470) from the fifth of the periods ROUGH_T on, beside an ordinary gradient"""
    vel = np.zeros((len(ROUGH_DEPZ), 1, 2), np.float32)
    vel[:, 0, 0] = [4.54608, 2.8430116, 3.6760201, 3.927757, 4.495318, 3.0541914, 3.4480517, 2.64218, 3.828745, 4.2]
    vel[:, 0, 1] = 3.0 + 0.02 * ROUGH_DEPZ
    return vel


def test_root_failure_is_reported(ctx, orc):
    """a column whose search leaves the window before the sign changes has no fundamental-mode root there: the reference returns
    cg=0 for the remaining periods (inv/surfdisp96.f:342-348).  The oracle loses the last four of the eight periods of column 0
    (the column this test used before, a half-space slower than the layers above it, lost none: 0 == 0)"""
    vel = no_root_column()
    pv, _, nf = ctx.depthkernel(vel, ROUGH_DEPZ, ROUGH_T, 3.0, kernels=False)
    pvo, _ = orc.depthkernel(vel, ROUGH_DEPZ, ROUGH_T, 3.0, kernels=False)
    assert int((pvo == 0).sum()) == 4 and (pvo[4:, 0] == 0).all() and (pvo[:, 1] > 0).all()
    assert nf > 0
    assert np.array_equal(pv == 0, pvo == 0)
    assert nf == int((pvo == 0).sum())
    within("root-failure columns pvRc max |d| km/s", np.abs(pv - pvo).max(), PV_ABS)


@pytest.mark.parametrize("sublayers", [2.0, 3.0, 4.0])
def test_division_free_sublayer_interpolation_is_exact(ctx, sublayers):
    """The sub-layer interpolation divides by 2*nsublay (inv/CalSurfG.f90:2352).  sublayers=3 -> 8: the kernel multiplies by
    1/8 (exact for a power of two); sublayers=2, 4 -> 6, 10: reciprocal + one fused correction step, which equals the
    correctly rounded quotient for those divisors (verified exhaustively over all floats in 1e-30..1e30).  Either way the
    results must be bit-identical to the dividing kernel (option disp.rden=0)."""
    depz = np.arange(12, dtype=np.float32) * 5.0
    vel = model(5, 4, depz, 7)
    t = np.arange(5, 37, 2, dtype=np.float64)
    pv1, sen1, nf1 = ctx.depthkernel(vel, depz, t, sublayers)
    ctx.set_option("disp.rden", 0)
    try:
        pv0, sen0, nf0 = ctx.depthkernel(vel, depz, t, sublayers)
    finally:
        ctx.set_option("disp.rden", 1)
    assert nf0 == nf1 and np.array_equal(pv0, pv1)
    for a, b in zip(sen0, sen1):
        assert np.array_equal(a, b)


def test_period_chunked_task_queue_is_bit_identical(orc):
    """option disp.pchunk: the periods of a work item handed from task to task (state = last root, del1st, fail flag in HBM,
    workgroups synchronised through release/acquire flags) must give exactly the unchunked results"""
    import dazimsurftomo_amd as dz
    depz = np.array([0.0, 4.0, 10.0, 18.0, 30.0, 45.0, 60.0], np.float32)
    vel = model(21, 19, depz, 11)
    t = np.arange(4.0, 41.0, 3.0)
    base = None
    for pc in (0, 1, 3, 5):
        c = dz.Context(0)
        if pc:
            c.set_option("disp.pchunk", pc)
        pv, sen, nf = c.depthkernel(vel, depz, t, 2.0)
        c.close()
        if base is None:
            base = (pv, sen, nf)
        else:
            assert nf == base[2] and np.array_equal(pv, base[0])
            for a, b in zip(sen, base[1]):
                assert np.array_equal(a, b)


def test_first_period_fast_forward_is_bit_identical(ctx):
    """The first period's bracket search jumps to the bracket that disp_bracket_kernel found for the column's own model by
    evaluating every grid point (exact for the column; the perturbed copies land 0.02 km/s below it, check the sign and fall
    back to the step-by-step search if it changed).  Results must equal those of the step-by-step search (option disp.ffwd = 0)
    bit for bit: ordinary columns, a deep model, a low-velocity zone with reversed dispersion, and a column without a root."""
    cases = []
    depz = np.arange(12, dtype=np.float32) * 5.0
    cases.append((model(9, 7, depz, 5), depz, np.arange(5, 37, 2, dtype=np.float64), 3.0))
    depz = np.array([0, 3, 6, 9, 12, 16, 20, 25, 30, 35, 40, 50, 60, 70, 80, 100, 120, 150], np.float32)
    cases.append((model(4, 3, depz, 6), depz, np.arange(5, 41, dtype=np.float64), 4.0))
    depz = np.array([0.0, 5.0, 10.0, 20.0, 35.0, 60.0], np.float32)
    vel = np.zeros((6, 2, 3), np.float32)
    vel[:] = np.array([3.4, 3.6, 2.9, 3.2, 3.9, 4.4], np.float32)[:, None, None]
    vel[:, 1, :] *= np.float32(1.03)
    cases.append((vel, depz, np.arange(4, 44, 2, dtype=np.float64), 3.0))
    depz = np.array([0.0, 10.0, 20.0, 40.0], np.float32)
    vel = np.zeros((4, 1, 2), np.float32)
    vel[:, 0, 0] = [3.0, 3.5, 3.9, 4.3]
    vel[:, 0, 1] = [4.6, 4.4, 3.0, 2.6]
    cases.append((vel, depz, np.array([5.0, 10.0, 20.0, 40.0, 60.0]), 2.0))
    for vel, depz, t, minthk in cases:
        for kernels in (True, False):
            _same_with_and_without_jump(ctx, vel, depz, t, minthk, kernels=kernels)


def _same_with_and_without_jump(ctx, vel, depz, t, minthk, kernels=True):
    """disp.ffwd = 1 (default: the column's own model jumps, exact by construction) and = 2 (opt-in: the perturbed copies jump too,
    behind the gates) against = 0 (step by step), bit for bit"""
    out = {}
    try:
        for mode in (0, 1, 2):
            ctx.set_option("disp.ffwd", mode)
            out[mode] = ctx.depthkernel(vel, depz, t, minthk, kernels=kernels)
            assert ctx.kernel_seconds("disp.ffwd_mode") == mode
            if mode == 2 and kernels:
                jumped, back = ctx.kernel_seconds("disp.ffwd_jumped_copies"), ctx.kernel_seconds("disp.ffwd_fallback_copies")
                assert 0 <= back <= jumped <= vel.shape[1] * vel.shape[2] * 6 * vel.shape[0]
    finally:
        ctx.set_option("disp.ffwd", 1)
    pv0, sen0, nf0 = out[0]
    for mode in (1, 2):
        pv1, sen1, nf1 = out[mode]
        assert nf0 == nf1 and np.array_equal(pv0, pv1), mode
        if kernels:
            for a, b in zip(sen0, sen1):
                assert np.array_equal(a, b), mode
    return pv0


ROUGH_DEPZ = np.array([0.0, 4.0, 9.0, 15.0, 22.0, 30.0, 40.0, 52.0, 66.0, 80.0], np.float32)
ROUGH_T = np.array([4.0, 6.0, 9.0, 13.0, 18.0, 25.0, 33.0, 42.0])


@pytest.mark.parametrize("seed", [101, 202, 303, 404, 505, 606, 707, 808])
def test_first_period_fast_forward_on_rough_random_models(ctx, seed):
    """1 200 columns per seed whose knots are drawn independently (Vs 2.6 .. 4.7 km/s, no smoothness, velocity inversions
    everywhere -- far rougher than anything an inversion produces).  Their secular functions have dips that touch zero and
    needle-like features narrower than the search step, where a 0.5 % change of one knot creates roots the column itself does
    not have: the jump of the perturbed copies is limited in front of a dip of the column's |del| and switched off for columns
    with a knot more than 25 % slower than one above it (disp_bracket_kernel), so the results must equal the step-by-step
    search's exactly -- phase velocities, depth kernels and failure count (rough columns have some failures).  Without the two
    safeguards 0.3 % of such columns differ (seed 101: columns 31, 801, 903, 1136; with the dip guard alone: column 996)."""
    rng = np.random.default_rng(seed)
    nx, ny = 40, 30
    vel = rng.uniform(2.6, 4.7, (len(ROUGH_DEPZ), ny, nx)).astype(np.float32)
    vel[-1] = np.maximum(vel[-1], 4.2)        # a fast half-space, so that most columns have a fundamental mode at all
    pv = _same_with_and_without_jump(ctx, vel, ROUGH_DEPZ, ROUGH_T, 3.0)
    assert (pv > 0).mean() > 0.5


@pytest.mark.parametrize("p", [0.05, 0.12])
def test_first_period_fast_forward_on_graded_random_models(ctx, p):
    """2 400 columns of a gradient 3.0 + 0.02 z km/s whose knots are perturbed independently by up to +-p (p = 12 %: velocity
    decreases of up to ~19 % below a shallower knot, twice what the bench model or the Yunnan example hold): here the jump is
    active for the perturbed copies, and must still give the step-by-step results bit for bit"""
    rng = np.random.default_rng(int(p * 1000))
    nx, ny = 60, 40
    base = (3.0 + 0.02 * ROUGH_DEPZ)[:, None, None]
    vel = (base * (1 + rng.uniform(-p, p, (len(ROUGH_DEPZ), ny, nx)))).astype(np.float32)
    _same_with_and_without_jump(ctx, vel, ROUGH_DEPZ, ROUGH_T, 3.0)


def test_phase_velocities_on_rough_random_columns(ctx, orc):
    """600 of the rough random columns (knots drawn independently from 2.6 .. 4.7 km/s) against the oracle, phase velocities only:
    their own bars (twice the measured 2.9e-6 km/s / 0.4 %) and the same root failures"""
    rng = np.random.default_rng(5)
    vel = rng.uniform(2.6, 4.7, (len(ROUGH_DEPZ), 20, 30)).astype(np.float32)
    vel[-1] = np.maximum(vel[-1], 4.2)
    pv, _, nf = ctx.depthkernel(vel, ROUGH_DEPZ, ROUGH_T, 3.0, kernels=False)
    pvo, _ = orc.depthkernel(vel, ROUGH_DEPZ, ROUGH_T, 3.0, kernels=False)
    assert np.array_equal(pv == 0, pvo == 0) and nf == int((pvo == 0).sum())
    within("rough random columns pvRc max |d| km/s", np.abs(pv - pvo).max(), PV_ABS_ROUGH)
    at_least("rough random columns pvRc bit-equal share", (pv == pvo).mean(), PV_EQUAL_SHARE_ROUGH)


def test_first_period_fast_forward_on_the_example_models(ctx):
    """the jump (both modes) on the model families of the bundled examples: the Yunnan starting model of test4 (18 knots, 86
    layers), the +-8 % checkerboards of test1-3 and a family of low-velocity zones of growing depth and strength"""
    import os
    g4 = os.path.join(os.path.dirname(__file__), "golden", "test4_yunnan.npz")
    if os.path.exists(g4):
        d = np.load(g4)
        vel = np.ascontiguousarray(d["vel"][:, ::3, ::3])
        _same_with_and_without_jump(ctx, vel, d["depz"], d["t"], float(d["minthk"]))
    a = np.load(os.path.join(os.path.dirname(__file__), "golden", "test1_authors.npz"))
    _same_with_and_without_jump(ctx, np.ascontiguousarray(a["vel"]), a["depz"], np.arange(5, 41, dtype=np.float64), 2.0)
    depz = np.array([0.0, 4.0, 8.0, 12.0, 18.0, 25.0, 35.0, 50.0, 70.0], np.float32)
    base = np.array([3.1, 3.3, 3.45, 3.55, 3.7, 3.85, 4.1, 4.35, 4.5], np.float32)
    vel = np.zeros((len(depz), 6, 8), np.float32)
    for j in range(6):          # position of the zone
        for i in range(8):      # its strength: 0 .. 21 % slower than the background
            v = base.copy()
            v[1 + j] *= np.float32(1.0 - 0.03 * i)
            v[2 + j] *= np.float32(1.0 - 0.02 * i)
            vel[:, j, i] = v
    _same_with_and_without_jump(ctx, vel, depz, np.arange(4, 40, 3, dtype=np.float64), 3.0)


def test_three_exponentials_option(ctx, orc):
    """option disp.exp3 = 1: exp(-2p), exp(-2q), exp(-(p+q)) by three exp() calls as in the reference's var (inv/surfdisp96.f:893,
    :927,:951) instead of ep*ep, eq*eq, ep*eq from two: the same roots after fp32 rounding on these models, both ways equal to
    the oracle's within the bars"""
    depz = np.arange(12, dtype=np.float32) * 5.0
    vel = model(6, 5, depz, 12)
    t = np.arange(5, 37, 2, dtype=np.float64)
    pv2, sen2, _ = ctx.depthkernel(vel, depz, t, 3.0)
    try:
        ctx.set_option("disp.exp3", 1)
        pv3, sen3, _ = ctx.depthkernel(vel, depz, t, 3.0)
    finally:
        ctx.set_option("disp.exp3", 0)
    pvo, seno = orc.depthkernel(vel, depz, t, 3.0)
    for pv, sen, tag in ((pv2, sen2, "two exp"), (pv3, sen3, "three exp")):
        within(f"pvRc max |d| km/s ({tag})", np.abs(pv - pvo).max(), PV_ABS)
        at_least(f"pvRc bit-equal share ({tag})", (pv == pvo).mean(), PV_EQUAL_SHARE)
        for a, b in zip(sen, seno):
            within(f"sen max |d| ({tag})", np.abs(a - b).max(), SEN_REL * np.abs(b).max() + SEN_ABS)


def test_two_stream_dispersion_is_bit_identical_and_joined_by_its_consumers():
    """option disp.async (device-resident arrays): the column curves on the context's stream, the 6*nz perturbed copies on the
    auxiliary stream, the call returns when the curves are there.  pvRc must be complete at once (the eikonal solve is next),
    the depth kernels after dazim_sync -- bit-identical to the one-stream call -- and dazim_rays_build_G must join the auxiliary
    stream by itself: the G built right after an asynchronous call equals the G of the one-stream call, entry for entry."""
    import torch
    import dazimsurftomo_amd as dz
    import bench
    from tests import synth
    dev = torch.device("cuda:0")
    nx = ny = 28
    old = (bench.NX, bench.NY)
    bench.NX = bench.NY = nx
    try:
        vel = bench.s256_model()
    finally:
        bench.NX, bench.NY = old
    depz, periods, minthk = bench.DEPZ, np.asarray(bench.PERIODS, np.float64)[:8], bench.MINTHK
    kmax, nsrc, nrcv = len(periods), 12, 8
    lat, lon = synth.stations(nx, ny, 30.0, 100.0, 0.25, 0.25, nsrc, seed=3)
    sx, sz = synth.radians(lat, lon)
    rlat, rlon = synth.stations(nx, ny, 30.0, 100.0, 0.25, 0.25, nrcv, seed=4)
    rx, rz = synth.radians(rlat, rlon)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_vel = T(vel)
    d_scx, d_scz = T(np.tile(sx, kmax)), T(np.tile(sz, kmax))
    d_per = T(np.repeat(np.arange(1, kmax + 1, dtype=np.int32), nsrc))
    nfield = kmax * nsrc
    d_fray = T(np.repeat(np.arange(nfield, dtype=np.int32), nrcv))
    d_rcx, d_rcz = T(np.tile(rx, nfield)), T(np.tile(rz, nfield))
    res = {}
    for mode in (0, 1, 1):
        c = dz.Context(0)
        c.set_option("disp.async", 2 * mode)
        pv, sen, nf = c.depthkernel(d_vel, depz, periods, minthk)
        assert c.kernel_seconds("disp.async") == mode
        pv_now = pv.clone()                                   # (on torch's stream, after the call returned: complete by contract)
        fields = c.fmm_batch(nx, ny, 30.0, 100.0, 0.25, 0.25, pv, d_scx, d_scz, d_per,
                             veln=torch.empty((kmax, 126, 126), dtype=torch.float32, device=dev),
                             ttn=torch.empty((nfield, 126, 126), dtype=torch.float32, device=dev),
                             ttnr=torch.empty((nfield, 129, 129), dtype=torch.float32, device=dev),
                             nstsr=torch.empty((nfield, 129, 129), dtype=torch.int32, device=dev),
                             boxes=torch.empty((nfield, 12), dtype=torch.int32, device=dev),
                             status=torch.empty((nfield,), dtype=torch.int32, device=dev))
        G, tpred, nb = c.rays_build_G(nx, ny, 30.0, 100.0, 0.25, 0.25, d_vel, fields, d_scx, d_scz, d_per, d_fray, d_rcx, d_rcz, sen)
        rowptr, col, val = G.to_coo()
        c.sync()
        if mode:
            assert c.kernel_seconds("disp.copies") > 0
        out = (pv_now.cpu().numpy(), [s.cpu().numpy() for s in sen], nf, rowptr, col, val, tpred.cpu().numpy())
        G.free()
        c.close()
        if mode == 0:
            res = out
        else:
            assert out[2] == res[2] and np.array_equal(out[0], res[0])
            for a, b in zip(out[1], res[1]):
                assert np.array_equal(a, b)
            for a, b in zip(out[3:], res[3:]):
                assert np.array_equal(a, b)


def test_column_curves_in_teams_are_bit_identical():
    """disp.async with the columns' own curves searched in teams (16 lanes per column, 16 grid points of the bracket search at
    a time, disp.team = 1) against the one-stream, one-lane-per-item search: pvRc, failures and depth kernels bit for bit on
    ordinary columns, a deep 18-knot model with 36 periods, a low-velocity zone with reversed dispersion (the search runs
    downwards and is turned round at its lower bound), a column without a root (bound violation before any sign change), and
    columns whose knots are drawn independently at random"""
    import torch
    import dazimsurftomo_amd as dz
    dev = torch.device("cuda:0")
    cases = []
    depz = np.arange(12, dtype=np.float32) * 5.0
    cases.append((model(9, 7, depz, 5), depz, np.arange(5, 37, 2, dtype=np.float64), 3.0))
    depz = np.array([0, 3, 6, 9, 12, 16, 20, 25, 30, 35, 40, 50, 60, 70, 80, 100, 120, 150], np.float32)
    cases.append((model(6, 5, depz, 6), depz, np.arange(5, 41, dtype=np.float64), 4.0))
    depz = np.array([0.0, 5.0, 10.0, 20.0, 35.0, 60.0], np.float32)
    vel = np.zeros((6, 2, 3), np.float32)
    vel[:] = np.array([3.4, 3.6, 2.9, 3.2, 3.9, 4.4], np.float32)[:, None, None]
    vel[:, 1, :] *= np.float32(1.03)
    cases.append((vel, depz, np.arange(4, 44, 2, dtype=np.float64), 3.0))
    depz = np.array([0.0, 10.0, 20.0, 40.0], np.float32)
    vel = np.zeros((4, 1, 2), np.float32)
    vel[:, 0, 0] = [3.0, 3.5, 3.9, 4.3]
    vel[:, 0, 1] = [4.6, 4.4, 3.0, 2.6]
    cases.append((vel, depz, np.array([5.0, 10.0, 20.0, 40.0, 60.0]), 2.0))
    rng = np.random.default_rng(4242)
    cases.append((rng.uniform(2.6, 4.7, (len(ROUGH_DEPZ), 20, 30)).astype(np.float32), ROUGH_DEPZ, ROUGH_T, 2.0))
    for vel, depz, t, minthk in cases:
        d_vel = torch.from_numpy(np.ascontiguousarray(vel)).to(dev)
        out = {}
        for mode in (0, 1):
            c = dz.Context(0)
            if mode:
                c.set_option("disp.async", 2)
                c.set_option("disp.team", 1)
            pv, sen, nf = c.depthkernel(d_vel, depz, t, minthk)
            if mode:
                assert c.kernel_seconds("disp.async") == 1 and c.kernel_seconds("disp.team") == 16
            pv_now = pv.clone()
            c.sync()
            out[mode] = (pv_now.cpu().numpy(), [s.cpu().numpy() for s in sen], nf)
            c.close()
        assert out[0][2] == out[1][2] and np.array_equal(out[0][0], out[1][0]), (vel.shape, np.abs(out[0][0] - out[1][0]).max())
        for a, b in zip(out[0][1], out[1][1]):
            assert np.array_equal(a, b)


FASTDIV_DENOMINATORS = (6, 10, 12, 14, 18, 20, 22, 24, 26, 28, 30, 36)   # the divisors the reciprocal + correction form was verified on


def _division_class(depz, sublayers, rden_option=1):
    """the kernel class (template argument RDEN) the driver picks: the 2*nsub of refineGrid2LayerMdl with the driver's fp32
    expressions; 1 = all powers of two, 2 = powers of two or verified divisors, 0 = divide (or option disp.rden = 0)"""
    depz = np.asarray(depz, np.float32)
    thk = depz[1:] - depz[:-1]
    minthk = thk / np.float32(sublayers)
    den = 2 * (((thk + np.float32(1.0e-4)) / minthk).astype(np.int64) + 1)
    assert thk.dtype == np.float32 and minthk.dtype == np.float32
    if rden_option == 0:
        return 0, den
    pow2 = (den & (den - 1)) == 0
    if pow2.all():
        return 1, den
    return (2 if (pow2 | np.isin(den, FASTDIV_DENOMINATORS)).all() else 0), den


def test_every_dispersion_kernel_form_gives_the_same_bits():
    """The driver launches one of four kernels per division class (RDEN 0, 1, 2): the plain form, the team form (the columns' own
    curves of a two-stream call), the form with shared layer stacks (the perturbed copies) and the first-period bracket kernel.
    Each class is run (a) plain on every variant, one stream, (b) with the defaults (shared stacks), (c) on two streams with the
    curves in teams and (d) as (a) without the bracket kernel: pvRc, the three kernel tables and the failure count must be the
    same bits in all four, class 0 (option disp.rden = 0) must equal class 2 on the same model, and the same model passed as host
    arrays declines the second stream and equals (a)."""
    import torch
    import dazimsurftomo_amd as dz
    dev = torch.device("cuda:0")
    depz = np.array([0.0, 5.0, 10.0, 20.0, 35.0, 60.0], np.float32)
    t = np.array([5.0, 8.0, 12.0, 18.0, 26.0, 36.0])
    vel = model(5, 4, depz, 21)
    d_vel = torch.from_numpy(np.ascontiguousarray(vel)).to(dev)

    def call(v, opts, want):
        c = dz.Context(0)
        try:
            for k, o in opts.items():
                c.set_option(k, o)
            pv, sen, nf = c.depthkernel(v, depz, t, sublayers)
            for k, w in want.items():
                assert c.kernel_seconds(k) == w, (cls, opts, k, c.kernel_seconds(k))
            c.sync()
            if isinstance(pv, torch.Tensor):
                pv, sen = pv.cpu().numpy(), [s.cpu().numpy() for s in sen]
            return pv, sen, nf
        finally:
            c.close()

    def same(x, y, what):
        assert x[2] == y[2], (what, x[2], y[2])
        assert np.array_equal(x[0], y[0]), (what, "pvRc", np.abs(x[0] - y[0]).max())
        for q, (a, b) in enumerate(zip(x[1], y[1])):
            assert np.array_equal(a, b), (what, "sen", q, np.abs(a - b).max())

    by_class = {}
    for cls, sublayers, rden, den_want in ((1, 3.0, 1, 8), (2, 2.0, 1, 6), (0, 2.0, 0, 6)):
        got, den = _division_class(depz, sublayers, rden)
        assert got == cls and (den == den_want).all(), (cls, got, den)
        base = {"disp.rden": 0} if rden == 0 else {}
        plain = dict(base, **{"disp.share": 0})
        a = call(d_vel, plain, {"disp.share": 0, "disp.async": 0, "disp.ffwd_mode": 1})
        b = call(d_vel, base, {"disp.share": 1, "disp.async": 0})
        c2 = call(d_vel, dict(base, **{"disp.async": 2, "disp.team": 1}), {"disp.async": 1, "disp.team": 16, "disp.share": 1})
        d = call(d_vel, dict(plain, **{"disp.ffwd": 0}), {"disp.share": 0, "disp.async": 0, "disp.ffwd_mode": 0})
        host = call(vel, dict(base, **{"disp.async": 2}), {"disp.async": 0})   # (staged buffers decline the second stream)
        assert (a[0] > 0).all() and a[2] == 0 and all(np.abs(s).max() > 0 for s in a[1])   # (a real answer, not equal garbage)
        same(b, a, (cls, "shared stacks"))
        same(c2, a, (cls, "two streams, teams"))
        same(d, a, (cls, "no fast-forward"))
        same(host, a, (cls, "host arrays"))
        by_class[cls] = a
    same(by_class[0], by_class[2], "dividing class against reciprocal + correction")


@pytest.mark.gpu
def test_host_copies_join_the_perturbed_copies_only_when_they_touch_their_arrays():
    """dazim_memcpy_h2d / _d2h after an asynchronous dazim_dispersion_kernels call: a copy into an unrelated device array leaves
    the auxiliary stream alone (the overlap with the eikonal solve survives staging the next inputs); a copy out of a kernel table
    or into the model waits for the copies first and delivers the finished table."""
    import ctypes
    import torch
    import dazimsurftomo_amd as dz
    import bench
    dev = torch.device("cuda:0")
    nx = ny = 28
    old = (bench.NX, bench.NY)
    bench.NX = bench.NY = nx
    try:
        vel = bench.s256_model()
    finally:
        bench.NX, bench.NY = old
    depz, periods, minthk = bench.DEPZ, np.asarray(bench.PERIODS, np.float64)[:8], bench.MINTHK
    d_vel = torch.from_numpy(np.ascontiguousarray(vel)).to(dev)
    ref = dz.Context(0)
    _, sen_ref, _ = ref.depthkernel(d_vel, depz, periods, minthk)
    ref.sync()
    want = sen_ref[0].cpu().numpy()
    ref.close()
    c = dz.Context(0)
    c.set_option("disp.async", 2)
    pv, sen, nf = c.depthkernel(d_vel, depz, periods, minthk)
    assert c.kernel_seconds("disp.async") == 1 and c.stat("aux.pending") == 1
    lib = c.lib
    lib.dazim_memcpy_h2d.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.dazim_memcpy_d2h.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    other = torch.zeros(1024, dtype=torch.float32, device=dev)
    src = np.arange(1024, dtype=np.float32)
    assert lib.dazim_memcpy_h2d(c._h, other.data_ptr(), src.ctypes.data, src.nbytes) == 0
    assert c.stat("aux.pending") == 1                       # unrelated array: not joined
    assert np.array_equal(other.cpu().numpy(), src)
    got = np.empty_like(want)
    assert lib.dazim_memcpy_d2h(c._h, got.ctypes.data, sen[0].data_ptr(), got.nbytes) == 0
    assert c.stat("aux.pending") == 0                       # a kernel table: joined, and complete
    assert np.array_equal(got, want)
    c.sync()
    c.close()

