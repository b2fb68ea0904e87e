"""-m gpu: the two views of tradeoff.hip feed one sweep.  A map problem of one period has the column layout blk * ncell + cell of a joint
3-D model of one knot layer (nz = 2), so the same matrix and right-hand side go through dazim_map_tradeoff (MtPeriod: row lists,
mp_accum_rows) and through dazim_model_tradeoff (MtModel: the transpose, mo_accum_row).

logdet_a, logdet_p and dof depend on W alone.  Both Gram routes add r_a r_c to an element once per row, rows ascending, from zero, and
both combine passes add s_b^2 (r_a r_c) in that order to D's element and d^2 to the diagonal; factor, inverse and the fixed-order sums
are the same launches.  So these three are equal bit for bit.  chi2, reg2, xnorm2, x and logev pass through g, which the model sums
over strided lanes and a butterfly and the maps in list order: they are held to the 1e-6 bar of the entries' own tests."""
import numpy as np
import pytest

from tests import map_posterior_ref as mref
from tests import map_tradeoff_ref as ref
from tests import model_tradeoff_ref as tref
from tests import test_map_tradeoff_gpu as mpt
from tests.bars import within

pytestmark = pytest.mark.gpu

W_ALONE = ("logdet_a", "logdet_p", "dof")
THROUGH_G = ("chi2", "reg2", "xnorm2", "x", "logev")
POINTS = [0, 16, 29]   # of ref.sweep: every block at 0.25 and half the damping; a1/a2 alone at 0.5; a1/a2 alone at 4 and twice the damping


def test_one_period_of_the_maps_is_a_joint_model_of_one_layer(ctx):
    """n = 45 (nx, ny = 7, 5, azim, kmax 1), K = 3, dof and evidence on: logdet_a, logdet_p and dof of the two entries are the same bits,
    the outputs that pass through g agree within 1e-6 * max(1, max |value|), nothing failed"""
    nx, ny = 7, 5
    prob = ref.problem(nx, ny, 1, True, mref.REGS[0])
    scale, damp = ref.sweep(prob)
    scale, damp = scale[POINTS].copy(), damp[POINTS].copy()
    assert prob["n"] == 45 and scale.shape == (3, 3)
    A = mpt.matrix(ctx, prob)
    maps = ctx.map_tradeoff(A, prob["m_data"], prob["b"], nx, ny, 1, True, scale, damp, dof=True, evidence=True, x=True)
    model = ctx.model_tradeoff(A, prob["m_data"], prob["b"], nx, ny, 2, True, scale, damp, dof=True, evidence=True, x=True)
    A.free()
    assert not maps["n_failed"].any() and not model["n_failed"].any() and maps["mdata_p"][0] == prob["m_data"]
    for k in W_ALONE:
        assert np.isfinite(model[k]).all(), k
        assert np.array_equal(mpt.bits(maps[k]).reshape(-1), mpt.bits(model[k]).reshape(-1)), k
    for k, v in tref.worst(maps, model, THROUGH_G).items():
        within(f"map_tradeoff vs model_tradeoff on one matrix, {k}", v, mpt.BAR)
