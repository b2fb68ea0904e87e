"""Worker of tests/test_matrix_lifecycle_gpu.py: `world` processes on ONE GPU over the file transport (dazim_comm_init_files).

    python tests/weights_shard_worker.py <rank> <world> <comm dir> <out.npz>

Every rank holds its slice [row0, row0 + dall) of one seeded list of observed and synthetic times and those rows of G, and calls
dazim_weight_data_sharded (Context.weight_data with row0 / dall_glob): the relative residuals of all ranks are put together inside
the library and every rank runs CalDdatSigma's two sequential sums over all of them.  The test wants the ranks' residuals,
weights, right-hand sides and scaled rows, put together, equal to the one-rank call's bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NDATA = 20877                                     # (test4_Yunnan's ray count: not a multiple of the 8192-entry chunk of k_sigma_stats)
CUTS = {2: [0, 9001, NDATA], 3: [0, 5000, 13193, NDATA]}      # uneven slices; 9001 and 13193 lie inside a chunk


def problem():
    """(obst, dsyn, Model of the NDATA x 12 data rows, three entries each)"""
    from tests.matrix_model import Model
    rng = np.random.default_rng(NDATA)
    obst = (20 + 80 * rng.random(NDATA)).astype(np.float32)
    dsyn = (obst * (1 + 0.02 * rng.standard_normal(NDATA))).astype(np.float32)
    dsyn[::17] *= np.float32(1.08)                # outliers: the exp() branch
    vals = rng.standard_normal(3 * NDATA).astype(np.float32)
    return obst, dsyn, Model(NDATA, 12, np.repeat(np.arange(NDATA), 3), np.tile([0, 3, 8], NDATA), vals)


def main(rank, world, comm_dir, out_path):
    import dazimsurftomo_amd as dz
    obst, dsyn, model = problem()
    lo, hi = CUTS[world][rank], CUTS[world][rank + 1]
    sel = (model.rows >= lo) & (model.rows < hi)
    ctx = dz.Context(0)
    ctx.comm_init_files(world, rank, comm_dir)
    G = ctx.csr_from_coo(hi - lo, model.n, (model.rows[sel] - lo + 1).astype(np.int32), (model.cols[sel] + 1).astype(np.int32),
                         model.vals[sel])
    # both products first: the transpose exists when the rows are scaled
    y = np.zeros(G.m, np.float32); ctx.aprod(1, G, np.ones(G.n, np.float32), y)
    x = np.zeros(G.n, np.float32); ctx.aprod(2, G, x, np.ones(G.m, np.float32))
    res, wgt, rhs, st = ctx.weight_data(G, obst[lo:hi], dsyn[lo:hi], row0=lo, dall_glob=NDATA)
    rw = G.to_coo()[2]
    # A^T 1 through the transpose that was there before the scaling, and on a matrix built afresh from the scaled rows
    xt = np.zeros(G.n, np.float32); ctx.aprod(2, G, xt, np.ones(G.m, np.float32))
    F = ctx.csr_from_coo(G.m, G.n, *G.to_coo())
    xf = np.zeros(G.n, np.float32); ctx.aprod(2, F, xf, np.ones(G.m, np.float32))
    F.free()
    G.free()
    ctx.comm_free()
    ctx.close()
    np.savez(out_path, res=res, wgt=wgt, rhs=rhs, rw=rw, xt=xt, xt_fresh=xf, stats=np.array(list(st.values()), np.float32), row0=lo, dall=hi - lo)


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4])
