"""-m gpu: dazim_dispersion_kernels_typed (csrc/disp_typed.hip) -- depthkernel for Rayleigh / Love, phase / group velocities in one
table over virtual periods -- on the common model of tests/typed_kernels_ref.py: 20 columns x 31 variants = 620 work items per
Rayleigh segment (420 per Love segment), i.e. more than one wavefront with the last one partial, wavefronts that span several
columns, a column with uniform Vs, one with a slow second knot, one with Vs falling with depth.

What is exact and what has a bar:
  * against depthkernel composed of dazim_surfdisp96 calls on host-built layer stacks (typed_kernels_ref driven by Context.surfdisp96):
    bit-equal, every table -- device against device, the same functions on the same layers.  This pins the lane / variant
    bookkeeping, the start-value chain across periods, the pairing of the -+ copies and the table layout;
  * the Rayleigh-phase slice against dazim_dispersion_kernels: bit-equal;
  * against the CPU oracle: the bars tests/test_surfdisp_full_gpu.py states for dazim_surfdisp96 against the oracle, pushed through
    the kernels' quotient (typed_kernels_ref.check_tables; tests/test_typed_kernels_ref_cpu.py shows the oracle is the reference).

Where this file departs from the issue that asked for it, and why.  The issue expected the uniform-Vs column to have no Love wave at
any period (zeros everywhere).  With iflsph = 1 the Earth flattening turns uniform Vs into a 0.5 % gradient over these 35 km, and the
reference finds a Love root at 6 and 12 s (3.4150, 3.4176 km/s) and none at 20 s; so does it for Vs falling with depth.  The case
the issue wants -- no root from some period on comes back as zeros and a count, not a fault or a NaN -- is therefore checked on the
entries where the reference's curves end: Love phase at the third period of both columns, Love group at the second period of the
falling one (pinned on the CPU by test_typed_kernels_ref_cpu.py).  Likewise the reference's own Love Vp kernel is not exactly 0 but
search noise (same CPU file); the library defines it as 0, and so does the yardstick."""
import ctypes as C

import numpy as np
import pytest

from tests import typed_kernels_ref as T

pytestmark = pytest.mark.gpu

OFF, K = T.offsets(T.SEGMENTS)
QN = ("sen_vs", "sen_vp", "sen_rho")


@pytest.fixture(scope="module")
def vel():
    return T.common_model()


@pytest.fixture(scope="module")
def dev(ctx, vel):
    """the four-segment call: (pv [K][ncol], sen 3 x [nz][K][ncol], n_failed)"""
    return ctx.dispersion_kernels_typed(vel, T.DEPZ, T.SEGMENTS, T.SUBLAYERS)


@pytest.fixture(scope="module")
def composed(ctx, vel):
    """the non-Rc segments as depthkernel composed of dazim_surfdisp96 calls (one batched call per segment)"""
    return T.typed_tables(vel, T.DEPZ, T.SUBLAYERS, T.SEGMENTS[1:], ctx.surfdisp96, batched=True)


def test_typed_segments_equal_depthkernel_composed_of_surfdisp96(dev, composed):
    pv, sen, _ = dev
    assert pv.shape == (K, T.NX * T.NY) and np.isfinite(pv).all() and all(np.isfinite(s).all() for s in sen)
    for (iw, ig, t), o in zip(T.SEGMENTS[1:], OFF[1:]):
        a, b = o, o + len(t)
        bad = np.argwhere(pv[a:b] != composed[0][a - OFF[1]:b - OFF[1]])
        assert len(bad) == 0, f"pv iwave={iw} igr={ig}: {len(bad)} entries differ, first (k, col) {bad[0]}"
        for q in range(3):
            bad = np.argwhere(sen[q][:, a:b] != composed[1][q][:, a - OFF[1]:b - OFF[1]])
            assert len(bad) == 0, f"{QN[q]} iwave={iw} igr={ig}: {len(bad)} entries differ, first (knot, k, col) {bad[0]}"
    assert (composed[1][0] != 0).mean() > 0.9            # (the comparison is not one of zeros)


def test_rayleigh_phase_slice_is_the_tuned_call(ctx, vel, dev):
    pv, sen, nf = dev
    k = len(T.SEGMENTS[0][2])
    pvr, senr, nfr = ctx.depthkernel(vel, T.DEPZ, T.SEGMENTS[0][2], T.SUBLAYERS)
    assert np.array_equal(pv[:k], pvr) and nfr == 0
    for q in range(3):
        assert np.array_equal(sen[q][:, :k], senr[q]), QN[q]
    # ... and a call whose only segment it is: that call, in all four tables
    pv1, sen1, nf1 = ctx.dispersion_kernels_typed(vel, T.DEPZ, T.SEGMENTS[:1], T.SUBLAYERS)
    assert np.array_equal(pv1, pvr) and nf1 == nfr
    for q in range(3):
        assert np.array_equal(sen1[q], senr[q]), QN[q]


def test_love_vp_kernel_is_zero_and_ended_curves_are_zeros_and_a_count(dev, composed, orc, vel):
    pv, sen, nf = dev
    assert not sen[1][:, OFF[2]:].any()                            # Love: no Vp sensitivity, exactly
    assert (sen[1][:, :OFF[2]] != 0).mean() > 0.9                  # (Rayleigh: there is one)
    # where the reference's curves end (oracle = reference: test_typed_kernels_ref_cpu.py)
    want = T.typed_tables(vel, T.DEPZ, T.SUBLAYERS, T.SEGMENTS, orc.surfdisp96_full)[0]
    ended = np.argwhere(want == 0)
    assert {tuple(e) for e in ended} == {(OFF[2] + 2, T.COL_UNIFORM), (OFF[2] + 2, T.COL_FALLING), (OFF[3] + 1, T.COL_FALLING)}
    assert np.array_equal(pv == 0, want == 0)
    for k, c in ended:
        assert pv[k, c] == 0.0 and all(not s[:, k, c].any() for s in sen)
    assert nf == len(ended) == int((composed[0] == 0).sum())       # (the Rayleigh-phase slice has no failed entry)
    for c in (T.COL_UNIFORM, T.COL_FALLING):
        assert (pv[:OFF[2], c] != 0).all() and (sen[0][:, :OFF[2], c] != 0).all()


def test_typed_segments_against_the_cpu_oracle(dev, orc, vel):
    pv, sen, _ = dev
    want = T.typed_tables(vel, T.DEPZ, T.SUBLAYERS, T.SEGMENTS[1:], orc.surfdisp96_full)
    T.check_tables("device vs oracle", (pv[OFF[1]:], [s[:, OFF[1]:] for s in sen]), want, vel, T.SEGMENTS[1:])


def test_arguments_are_checked(ctx, vel):
    t3 = np.array([6.0, 12.0, 20.0])
    bad = [
        [T.RG + (t3,), T.RG + (t3,)],                              # a repeated segment
        [T.RG + (np.zeros(0),)],                                   # seg_kmax 0
        [T.RG + (np.arange(1.0, 62.0),)],                          # seg_kmax 61 > NP
        [T.RC + (t3,), T.RG + (t3,), T.LC + (t3,), T.LG + (t3,), T.RG + (t3,)],   # nseg 5
        [(3, 0, t3)],                                              # iwave 3
        [(1, 2, t3)],                                              # igr 2
    ]
    for segs in bad:
        with pytest.raises(RuntimeError):
            ctx.dispersion_kernels_typed(vel, T.DEPZ, segs, T.SUBLAYERS)
    # only one of the three sen_* given
    nz, ncol = vel.shape[0], T.NX * T.NY
    iw, ig, km = (np.array([x], np.int32) for x in (2, 1, 3))
    pv, svs = np.zeros((3, ncol)), np.zeros((nz, 3, ncol))
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = ctx.lib.dazim_dispersion_kernels_typed(ctx._h, T.NX, T.NY, nz, p(vel), p(T.DEPZ), C.c_float(T.SUBLAYERS), 1, p(iw), p(ig), p(km), p(t3),
                                                p(pv), p(svs), None, None, None)
    assert rc != 0 and b"all three or none" in ctx.lib.dazim_last_error(ctx._h)


def test_a_segment_does_not_depend_on_its_neighbours(ctx, vel, dev):
    pv, sen, _ = dev
    segs = [T.SEGMENTS[1], T.SEGMENTS[2]]
    pv2, sen2, nf2 = ctx.dispersion_kernels_typed(vel, T.DEPZ, segs, T.SUBLAYERS)
    a, b = OFF[1], OFF[3]
    assert np.array_equal(pv2, pv[a:b]) and nf2 == int((pv[a:b] == 0).sum())
    for q in range(3):
        assert np.array_equal(sen2[q], sen[q][:, a:b]), QN[q]
    # curves only: the same pv, one lane per column
    pv3, none, nf3 = ctx.dispersion_kernels_typed(vel, T.DEPZ, T.SEGMENTS, T.SUBLAYERS, kernels=False)
    assert none is None and np.array_equal(pv3, pv) and nf3 == dev[2]


def test_device_resident_arrays_give_the_same_tables(ctx, vel, dev):
    import torch
    pv, sen, nf = dev
    pvt, sent, nft = ctx.dispersion_kernels_typed(torch.from_numpy(vel).cuda(), T.DEPZ, T.SEGMENTS, T.SUBLAYERS)
    ctx.sync()
    assert nft == nf and np.array_equal(pvt.cpu().numpy(), pv)
    for q in range(3):
        assert np.array_equal(sent[q].cpu().numpy(), sen[q]), QN[q]
