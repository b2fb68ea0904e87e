"""-m gpu: disp_kernel and disp_bracket_kernel (dazimsurftomo_amd/csrc/disp.hip) where surfdisp96's guards and its search switch --
the inputs of tests/disp_cases.py, which tests/test_disp_cases_cpu.py shows to take the saturated exponentials (p >= 16, q >= 16,
p + q >= 60), an oscillatory P part, the omega clamp, downward starts, Neville's bisection guards and the exit at betmx + dc
(tests/test_disp_gpu.py's inputs take none of the saturation branches), and the first periods at which the bracket kernel's
64-point blocks hand over.

The device is compared with the oracle (oracle/disp.c, which equals the compiled reference bit for bit on the recorded runs:
tests/golden/disp_stress.npz) within the layered-model bars of tests/test_disp_gpu.py, unchanged: pvRc to one fp32 ulp with 99.9 %
of the entries bit-equal, sen_* to 2e-5 absolute and 1e-6 relative L2.  Where the oracle's sen_* entry is an exact zero (a knot
the wave no longer reaches: cg2 == cg1 bit for bit, a third to three quarters of the entries here) the device must stay within
2e-5 and be an exact zero itself on 99.8 % of them (two curves, each held to the 99.9 % bit-equal share).  Every figure is printed
before it is asserted (pytest -s).

Measured on an MI355X ("Dispersion kernels where surfdisp96 saturates"): on every case pvRc and the three
tables are the oracle's bits (max |d| 0, every share 1.0), both exponential forms included; with disp.ffwd = 2 all 48 copies of
the planted column jump and none comes back for lower ends 62 .. 510, none jumps beyond.  The file takes 9.4 s, 7.5 s of them the
oracle's."""
import numpy as np
import pytest

from tests import disp_cases as D
from tests.bars import at_least, within
from tests.test_disp_gpu import PV_ABS, PV_EQUAL_SHARE, SEN_ABS, SEN_L2, _division_class

pytestmark = pytest.mark.gpu
CASES = D.cases()
ZERO_EQUAL_SHARE = 0.998     # two curves (cg1, cg2), each bit-equal to the oracle's on PV_EQUAL_SHARE of the entries


@pytest.fixture(scope="module")
def want(orc):
    """{name: (pv, sen)} of the oracle on every case, computed once and left alone"""
    out = {}
    for name, c in CASES.items():
        pv, sen = orc.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"], kernels=c["kernels"])
        pv.setflags(write=False)
        for s in sen or ():
            s.setflags(write=False)
        out[name] = (pv, sen)
    return out


def run(ctx, c, opts=None):
    """one call of the shared context with options set for the call only -> (pv, sen, nf)"""
    opts = opts or {}
    default = {"disp.exp3": 0, "disp.ffwd": 1, "disp.rden": 1, "disp.share": 1, "disp.pchunk": 0}
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        return ctx.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"], kernels=c["kernels"])
    finally:
        for k in opts:
            ctx.set_option(k, default[k])


@pytest.fixture(scope="module")
def got(ctx):
    """{name: (pv, sen, nf)} of the device with its defaults, computed lazily, once, and left alone"""
    cache = {}

    def get(name):
        if name not in cache:
            pv, sen, nf = run(ctx, CASES[name])
            pv.setflags(write=False)
            for s in sen or ():
                s.setflags(write=False)
            cache[name] = (pv, sen, nf)
        return cache[name]
    return get


def against_oracle(what, dev, ref):
    """the bars of tests/test_disp_gpu.py::compare, plus the failure mask, the exact zeros and finiteness"""
    (pv, sen, nf), (pvo, seno) = dev, ref
    assert pv.shape == pvo.shape and np.isfinite(pv).all(), what
    fails = int((pvo == 0).sum())
    print(f"\n[{what}] failures {nf} (oracle {fails} of {pvo.size})")
    assert np.array_equal(pv == 0, pvo == 0), (what, "failure mask", np.argwhere((pv == 0) != (pvo == 0)).tolist())
    assert nf == fails, (what, nf, fails)
    d, share = np.abs(pv - pvo).max(), (pv == pvo).mean()
    print(f"[{what}] pv max |d| {d:.2e} bit-equal {share:.5f}")
    within(f"{what}: pvRc max |d| km/s", d, PV_ABS)
    at_least(f"{what}: pvRc bit-equal share", share, PV_EQUAL_SHARE)
    if seno is None:
        assert sen is None
        return
    for name, a, b in zip(("vs", "vp", "rho"), sen, seno):
        assert a.shape == b.shape and np.isfinite(a).all(), (what, name)
        dmax, nb = np.abs(a - b).max(), np.linalg.norm(b)
        l2 = np.linalg.norm(a - b) / nb if nb > 0 else (0.0 if np.array_equal(a, b) else np.inf)
        zero = b == 0
        nzero = int(zero.sum())
        zmax = float(np.abs(a[zero]).max()) if nzero else 0.0
        zshare = float((a[zero] == 0).mean()) if nzero else 1.0
        print(f"[{what}] sen_{name}: max |d| {dmax:.2e} (max |sen| {np.abs(b).max():.2e}) rel-L2 {l2:.2e} bit-equal {(a == b).mean():.5f}; "
              f"oracle's exact zeros {nzero} of {b.size}: device max {zmax:.2e}, exact zeros {zshare:.5f}")
        within(f"{what}: sen_{name} max |d|", dmax, SEN_ABS)
        within(f"{what}: sen_{name} rel-L2", l2, SEN_L2)
        within(f"{what}: sen_{name} |device| where the oracle has an exact zero", zmax, SEN_ABS)
        at_least(f"{what}: sen_{name} share of the oracle's exact zeros that are exact zeros", zshare, ZERO_EQUAL_SHARE)


def same_bits(what, x, y):
    assert x[2] == y[2], (what, "nf", x[2], y[2])
    assert np.array_equal(x[0], y[0]), (what, "pvRc", np.abs(x[0] - y[0]).max())
    assert (x[1] is None) == (y[1] is None)
    for q, (a, b) in enumerate(zip(x[1] or (), y[1] or ())):
        assert np.array_equal(a, b), (what, "sen", q, np.abs(a - b).max())


# ---- the device against the oracle, every case ----
@pytest.mark.parametrize("name", list(CASES))
def test_device_against_the_oracle(got, want, name):
    if name in D.GOLDEN_KEYS:      # the compiled reference's own word: the same bits as the oracle's
        gold = np.load(D.GOLD)
        assert np.array_equal(want[name][0], gold[f"{name}_pv"])
        for q, s in zip(("vs", "vp", "rho"), want[name][1]):
            assert np.array_equal(s, gold[f"{name}_sen_{q}"])
    if name in D.STRESS_KEYS + ("B_2",):
        assert any((s == 0).mean() > 0.3 for s in want[name][1])       # (the knots the wave no longer reaches: exact zeros)
    against_oracle(name, got(name), want[name])


@pytest.mark.parametrize("name", D.EXP_KEYS)
def test_both_exponential_forms(ctx, got, want, name):
    """disp.exp3 = 1: exp(-2p), exp(-2q), exp(-(p+q)) by three exp() calls as the reference; 0: ep*ep, eq*eq, ep*eq from two.  The
    guards p < 16, q < 16, exa < 60 are where the two forms can part: each within the bars"""
    three = run(ctx, CASES[name], {"disp.exp3": 1})
    two = got(name)
    diff = [int((a != b).sum()) for a, b in zip((two[0],) + tuple(two[1]), (three[0],) + tuple(three[1]))]
    print(f"\n[{name}] entries that differ between the two forms (pv, sen_vs, sen_vp, sen_rho): {diff}")
    against_oracle(f"{name}, three exp", three, want[name])
    against_oracle(f"{name}, two exp", two, want[name])


# ---- every kernel form on saturated layers, bit for bit ----
@pytest.mark.parametrize("name", ["B_1", "B_2"])
def test_every_kernel_form_on_saturated_layers(got, want, name):
    """the plain form (one stream, no shared stacks) against shared stacks, two streams with teams on device tensors, the
    first-period jump off / on / on for the copies, period chunks, and at minthk 2 the dividing interpolation: the same pvRc,
    tables and failure count.  The options are read back, so a form that was declined cannot pass."""
    import torch
    import dazimsurftomo_amd as dz
    c = CASES[name]
    d_vel = torch.from_numpy(c["vel"]).cuda()

    def call(v, opts, report):
        x = dz.Context(0)
        try:
            for k, o in opts.items():
                x.set_option(k, o)
            pv, sen, nf = x.depthkernel(v, c["depz"], c["t"], c["minthk"])
            for k, w in report.items():
                assert x.kernel_seconds(k) == w, (name, opts, k, x.kernel_seconds(k))
            x.sync()
            if isinstance(pv, torch.Tensor):
                pv, sen = pv.cpu().numpy(), [s.cpu().numpy() for s in sen]
            return pv, sen, nf
        finally:
            x.close()

    plain = call(c["vel"], {"disp.share": 0}, {"disp.share": 0, "disp.async": 0, "disp.ffwd_mode": 1})
    against_oracle(f"{name}, plain form", plain, want[name])
    same_bits("defaults (shared stacks, the session's context)", got(name), plain)
    same_bits("shared stacks", call(c["vel"], {}, {"disp.share": 1, "disp.async": 0, "disp.ffwd_mode": 1}), plain)
    same_bits("device tensors", call(d_vel, {"disp.share": 0}, {"disp.share": 0, "disp.async": 0}), plain)
    same_bits("two streams, teams", call(d_vel, {"disp.async": 2, "disp.team": 1}, {"disp.async": 1, "disp.team": 16, "disp.share": 1}), plain)
    same_bits("two streams, teams, no shared stacks",
              call(d_vel, {"disp.async": 2, "disp.team": 1, "disp.share": 0}, {"disp.async": 1, "disp.team": 16, "disp.share": 0}), plain)
    for mode in (0, 2):
        for share in (0, 1):
            same_bits(f"disp.ffwd = {mode}, disp.share = {share}",
                      call(c["vel"], {"disp.ffwd": mode, "disp.share": share}, {"disp.ffwd_mode": mode, "disp.share": share}), plain)
    for share in (0, 1):      # (period chunks switch the jump off: that is how the call reports them)
        same_bits(f"disp.pchunk = 3, disp.share = {share}",
                  call(c["vel"], {"disp.pchunk": 3, "disp.share": share}, {"disp.ffwd_mode": 0, "disp.share": share}), plain)
    cls, den = _division_class(c["depz"], c["minthk"])
    if name == "B_2":       # 2 nsub = 6: reciprocal + correction (class 2); disp.rden = 0 divides (class 0)
        assert cls == 2 and (den == 6).all() and _division_class(c["depz"], c["minthk"], 0)[0] == 0
        for share in (0, 1):
            same_bits(f"disp.rden = 0, disp.share = {share}", call(c["vel"], {"disp.rden": 0, "disp.share": share}, {"disp.share": share}), plain)
    else:
        assert cls == 1 and (den == 4).all()


# ---- the bracket kernel's block edges ----
@pytest.mark.parametrize("name", D.FFWD_KEYS)
def test_bracket_kernel_edges(ctx, got, want, name):
    """the bracket's lower end at the last lanes of a block, at lane 0 of the next (sign and c carried from the block before), at
    the last point the kernel evaluates and beyond it; walks that end at betmx + dc inside a block; first periods without a root:
    disp.ffwd = 1 and 2 give the bits of the step-by-step search, which is held to the oracle.  The jump statistics show that the
    copies did jump where the kernel can find the bracket and did not where it cannot."""
    c = CASES[name]
    out = {}
    for mode in (0, 1, 2):
        out[mode] = run(ctx, c, {"disp.ffwd": mode})
        assert ctx.kernel_seconds("disp.ffwd_mode") == mode
        if mode == 2:
            jumped, back = ctx.kernel_seconds("disp.ffwd_jumped_copies"), ctx.kernel_seconds("disp.ffwd_fallback_copies")
            gated, dips = ctx.kernel_seconds("disp.ffwd_gated_columns"), ctx.kernel_seconds("disp.ffwd_dip_columns")
    ncopies = c["vel"].shape[1] * c["vel"].shape[2] * 6 * c["vel"].shape[0]
    print(f"\n[{name}] disp.ffwd = 2: {jumped:.0f} of {ncopies} copies jumped, {back:.0f} came back; gated columns {gated:.0f}, dips {dips:.0f}")
    against_oracle(f"{name}, step by step", out[0], want[name])
    same_bits(f"{name}: disp.ffwd = 1", out[1], out[0])
    same_bits(f"{name}: disp.ffwd = 2", out[2], out[0])
    same_bits(f"{name}: the session's first call", got(name), out[1])
    assert 0 <= back <= jumped <= ncopies
    if name.startswith("planted_"):
        # a copy's root lies within 0.5 % of c (0.0195 km/s at 3.9 km/s) of the column's, less than the 0.02 km/s the copies keep below
        # the column's bracket: where the kernel reports the bracket every jump arrives below the copy's root (none comes back),
        # and with the lower end carried wrongly from the block before none would jump (or all would come back)
        if int(name.split("_")[1]) in D.FOUND_BY_BRACKET_KERNEL:
            assert gated == 0
            assert jumped > 0 and back == 0, (name, jumped, back)
        else:
            assert jumped == 0, (name, jumped)
    if name in ("B_3_80first", "first_fails"):      # no sign change among the 512 points / before betmx + dc: nothing to jump to
        assert jumped == 0, (name, jumped)


# ---- shapes ----
def test_one_column_is_less_than_a_wavefront(ctx, got, want):
    c = CASES["planted_127"]
    assert c["vel"].shape == (8, 1, 1)          # 49 variants
    against_oracle("1 x 1 model", got("planted_127"), want["planted_127"])
    pv, sen, nf = run(ctx, dict(c, kernels=False))
    assert sen is None and nf == 0 and np.array_equal(pv, got("planted_127")[0])      # one lane


def test_65_columns_one_period(ctx, orc):
    """kmax = 1 and 65 columns: a wavefront and one lane of column curves, 65 blocks of the bracket kernel, on saturated layers"""
    rng = np.random.default_rng(65)
    vel = (D.planted_column()[:, 0, :1][:, None, :] * (1 + 0.02 * rng.standard_normal((8, 1, 65)))).astype(np.float32)
    for kernels in (False, True):
        c = D._case(vel, D.DEPZ, [1.0], 1.0, kernels=kernels)
        ref = orc.depthkernel(c["vel"], c["depz"], c["t"], c["minthk"], kernels=kernels)
        against_oracle(f"65 columns, kmax = 1, kernels = {kernels}", run(ctx, c), ref)
        same_bits("65 columns, step by step", run(ctx, c, {"disp.ffwd": 0}), run(ctx, c))


def test_scratch_reuse_across_shapes(ctx, got):
    """21 columns x 49 variants x 8 periods, then 1 x 1, then 3 columns x 25 variants that all fail, then the first again on one
    context: the named scratch buffers are reused with other strides and a failure count in between"""
    first = got("B_1")
    for other in ("planted_63", "first_fails", "B_1_long"):
        same_bits(other, run(ctx, CASES[other]), got(other))
        same_bits(f"B_1 after {other}", run(ctx, CASES["B_1"]), first)


def test_device_tensors_give_the_bits_of_host_arrays(ctx, got):
    import torch
    for name in ("B_0.5", "A_1_long"):
        c = CASES[name]
        pv, sen, nf = ctx.depthkernel(torch.from_numpy(c["vel"]).cuda(), c["depz"], c["t"], c["minthk"])
        ctx.sync()
        assert pv.is_cuda and all(s.is_cuda for s in sen)
        same_bits(name, (pv.cpu().numpy(), [s.cpu().numpy() for s in sen], nf), got(name))
