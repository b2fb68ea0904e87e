"""-m gpu: the shared layer stacks of the dispersion kernel (option disp.share, csrc/disp.hip: TableLayers) against the path that
rebuilds every layer from the knots at every secular evaluation (disp.share = 0).

The tables hold what layer_model returns and the lanes consume the values in the same place, so nothing may move: phase
velocities, the three depth-kernel tables and the failure count are compared BYTE FOR BYTE (no tolerance), on the bench models, a
model of the test4 kind (18 knots, 2 * nsublay = 10: the reciprocal + correction form of the interpolation), the bundled Yunnan
model, low-velocity zones, rough random columns (some without a root), a column without a root, with the two-stream launch, with
the periods handed from task to task, and with the first-period jump off and on for the perturbed copies.  A model whose
tables do not fit the LDS must report disp.share = 0 and still give the same results."""
import os

import numpy as np
import pytest

from tests.test_disp_gpu import ROUGH_DEPZ, ROUGH_T, model

pytestmark = pytest.mark.gpu

DEEP_DEPZ = np.array([0, 3, 6, 9, 12, 16, 20, 25, 30, 35, 40, 50, 60, 70, 80, 100, 120, 150], np.float32)


def _bench_model(workload):
    """bench.py's model of a workload; every module global of bench is put back (set_workload rewrites some of them)"""
    import bench
    old = {k: v for k, v in vars(bench).items() if k.isupper()}
    try:
        bench.set_workload(workload)
        return bench.s256_model(), bench.DEPZ.copy(), np.asarray(bench.PERIODS, np.float64).copy(), bench.MINTHK
    finally:
        for k, v in old.items():
            setattr(bench, k, v)


def _lvz_family():
    depz = np.array([0.0, 4.0, 8.0, 12.0, 18.0, 25.0, 35.0, 50.0, 70.0], np.float32)
    base = np.array([3.1, 3.3, 3.45, 3.55, 3.7, 3.85, 4.1, 4.35, 4.5], np.float32)
    vel = np.zeros((len(depz), 6, 8), np.float32)
    for j in range(6):          # position of the zone
        for i in range(8):      # its strength: 0 .. 21 % slower than the background
            v = base.copy()
            v[1 + j] *= np.float32(1.0 - 0.03 * i)
            v[2 + j] *= np.float32(1.0 - 0.02 * i)
            vel[:, j, i] = v
    return vel, depz, np.arange(4, 40, 3, dtype=np.float64), 3.0


def _rough(seed):
    rng = np.random.default_rng(seed)
    vel = rng.uniform(2.6, 4.7, (len(ROUGH_DEPZ), 20, 30)).astype(np.float32)
    vel[-1] = np.maximum(vel[-1], 4.2)
    return vel, ROUGH_DEPZ, ROUGH_T, 3.0


def _no_root():
    """a column whose search leaves the window from the fifth period on (a fast lid over slow channels: the reference returns 0
    for the remaining periods, inv/surfdisp96.f:342-348) beside an ordinary gradient"""
    vel = np.zeros((len(ROUGH_DEPZ), 1, 2), np.float32)
    vel[:, 0, 0] = [4.54608, 2.8430116, 3.6760201, 3.927757, 4.495318, 3.0541914, 3.4480517, 2.64218, 3.828745, 4.2]
    vel[:, 0, 1] = 3.0 + 0.02 * ROUGH_DEPZ
    return vel, ROUGH_DEPZ, ROUGH_T, 3.0


def _yunnan():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "test4_yunnan.npz"))
    return np.ascontiguousarray(d["vel"][:, ::2, ::2]), d["depz"], d["t"], float(d["minthk"])


MODELS = {
    "bench_s256": lambda: _bench_model("s256"),
    "bench_s128": lambda: _bench_model("s128"),
    "test4_kind": lambda: (model(9, 7, DEEP_DEPZ, 6), DEEP_DEPZ, np.arange(5, 41, dtype=np.float64), 4.0),
    "yunnan": _yunnan,
    "low_velocity_zones": _lvz_family,
    "rough_random": lambda: _rough(4242),
    "no_root": _no_root,
}


def _run(case, share, opts=(), device=False):
    """one call in a context of its own -> (bytes of pv, sen_vs, sen_vp, sen_rho, failure count, what disp.share reports)"""
    import dazimsurftomo_amd as dz
    vel, depz, t, minthk = case
    c = dz.Context(0)
    try:
        c.set_option("disp.share", share)
        for name, value in opts:
            c.set_option(name, value)
        if device:
            import torch
            d_vel = torch.from_numpy(np.ascontiguousarray(vel)).to("cuda:0")
            pv, sen, nf = c.depthkernel(d_vel, depz, t, minthk)
            pv = pv.clone()         # (complete when the call returns, also with disp.async; the depth kernels after the sync)
            c.sync()
            pv, sen = pv.cpu().numpy(), [s.cpu().numpy() for s in sen]
        else:
            pv, sen, nf = c.depthkernel(vel, depz, t, minthk)
        flag = c.kernel_seconds("disp.share")
        asyn = c.kernel_seconds("disp.async")
    finally:
        c.close()
    return [pv.tobytes()] + [s.tobytes() for s in sen], nf, flag, asyn


def _same(case, opts=(), device=False, want_async=None, shared=1):
    old, nf0, flag0, _ = _run(case, 0, opts, device)
    new, nf1, flag1, asyn = _run(case, 1, opts, device)
    assert flag0 == 0 and flag1 == shared, (flag0, flag1)
    if want_async is not None:
        assert asyn == want_async
    assert nf0 == nf1
    for name, a, b in zip(("pv", "sen_vs", "sen_vp", "sen_rho"), old, new):
        assert a == b, f"{name} differs between disp.share = 0 and 1"
    return nf1


@pytest.mark.parametrize("name", sorted(MODELS))
def test_shared_layers_are_byte_identical(name):
    """one launch for all variants of every column (host arrays): the column's own curve sits among its copies"""
    nf = _same(MODELS[name]())
    if name == "no_root":
        assert nf == 4       # (its last four periods: the failure path is compared too)
    if name == "rough_random":
        assert nf > 0        # (17 periods of 4 columns in the CPU restatement)


@pytest.mark.parametrize("name", ["bench_s128", "test4_kind", "rough_random"])
@pytest.mark.parametrize("asyn", [0, 2])
def test_shared_layers_with_and_without_the_two_stream_launch(name, asyn):
    """device arrays; disp.async = 2: the copies are a launch of their own (72 / 108 / 60 variants per column, no column curve
    among them) on the auxiliary stream and form the central differences themselves"""
    _same(MODELS[name](), opts=(("disp.async", asyn),), device=True, want_async=1 if asyn else 0)


@pytest.mark.parametrize("name", ["bench_s128", "test4_kind", "low_velocity_zones"])
def test_shared_layers_with_period_chunks(name):
    """disp.pchunk shorter than kmax: the tables are rebuilt by every task of an item's chain"""
    case = MODELS[name]()
    assert len(case[2]) > 3
    _same(case, opts=(("disp.pchunk", 3),))


@pytest.mark.parametrize("name", ["bench_s128", "test4_kind", "rough_random", "low_velocity_zones"])
@pytest.mark.parametrize("ffwd", [0, 2])
def test_shared_layers_with_the_first_period_jump_off_and_on_for_the_copies(name, ffwd):
    """disp.ffwd = 0 / 2: the start point of a jump is stashed in the lane's Neville table, which the sharing kernel keeps in HBM"""
    _same(MODELS[name](), opts=(("disp.ffwd", ffwd),))


def test_shared_layers_with_the_dividing_interpolation():
    """disp.rden = 0: the tables are built by the dividing form of the sub-layer interpolation"""
    _same(MODELS["test4_kind"](), opts=(("disp.rden", 0),))


def test_tables_that_do_not_fit_fall_back():
    """21 sublayers per interval (148 layers, a knot touches 42 of them): the patch tables alone would take 126 KB per
    workgroup -- the call must take the path that rebuilds its layers, say so, and give the same results"""
    depz = np.array([0.0, 6.0, 13.0, 21.0, 30.0, 42.0, 56.0, 75.0], np.float32)
    case = (model(5, 4, depz, 9), depz, np.arange(5, 35, 4, dtype=np.float64), 20.0)
    _same(case, shared=0)
    _same(case, opts=(("disp.async", 2),), device=True, want_async=1, shared=0)
