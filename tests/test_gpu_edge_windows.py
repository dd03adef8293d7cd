"""Refine windows and masks at the frame edge, per kernel family (tests/_edge_windows.py), on the
device.  Needs a real MI355X.

Pinned evaluation: with ``low = high = params`` no variable is free; the engine must return the
start bit for bit after one round with the reference objective there as its cost -- to rtol 1e-9
of NumPy's evaluation (gaussian families) or of the C oracle's pinned cost (lowpass, ring, disc,
inv_series, whose window and mask code the gaussian cells pin to NumPy on the CPU).  One wrong
pixel moves the cost by about 1 / (2 P) >= 1.9e-4 at the largest P here; reordered or contracted
float64 sums stay near 1e-13.  Status 1 and a NaN cost where no feature passes the filter or the
masks reach no pixel.

Well-posed clipped fits (faces, corners, a thin axis 0, every centre inside the frame): the engine
against the C oracle with the dispatch matrix's own assertion and tolerances."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _edge_windows as E
from test_gpu_dispatch_matrix import assert_engine_matches_oracle, std_from_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('cid', list(E.CELLS))
def test_pinned_evaluation(engine, oracle, cid):
    cell = E.CELLS[cid]
    worst, failures = 0., []
    for pl in E.placements(cid):
        problem = pl.prep().problem
        b = pl.pinned()
        engine.refine_batch(problem, b)
        if cell.family in E.GAUSS_FAMILIES:
            cost, _, status = E.numpy_yardstick(problem, b)
        else:
            ref = pl.pinned()
            oracle.run_batch(problem, ref)
            cost, status = ref.cost, ref.status
            assert_array_equal(ref.params_out, ref.params, err_msg=pl.id)
        assert set(status) <= {0, 1}, (pl.id, status)
        if pl.name.startswith(('all_filtered', 'kept_no_pixel')):
            assert (status == 1).all(), pl.id
        if pl.name.startswith(('inside', 'low', 'high', 'corner')):
            assert (status == 0).all(), pl.id     # (the yardstick itself: the oracle's, for some cells)
        ok = status == 0
        rel = np.abs(b.cost[ok] / cost[ok] - 1) if ok.any() else np.zeros(1)
        print('%s: status %s rounds %s iter %s worst relative cost difference %.2e'
              % (pl.id, sorted(set(b.status)), sorted(set(b.n_rounds)), sorted(set(b.n_iter)), np.nanmax(rel)))
        worst = max(worst, np.nanmax(rel))
        if not np.array_equal(b.status, status):
            failures.append((pl.id, 'status', b.status.tolist(), status.tolist()))
            continue
        if not (b.n_rounds[ok] == 1).all():
            failures.append((pl.id, 'n_rounds', b.n_rounds.tolist()))
        if not np.array_equal(b.params_out, b.params):
            failures.append((pl.id, 'params_out != params', float(np.abs(b.params_out - b.params).max())))
        if not np.isnan(b.cost[~ok]).all():
            failures.append((pl.id, 'cost where status 1', b.cost[~ok].tolist()))
        if not (rel <= 1e-9).all():     # (a NaN cost fails too)
            failures.append((pl.id, 'cost', float(np.nanmax(rel)), b.cost[ok].tolist(), cost[ok].tolist()))
    print('%s: worst relative cost difference %.2e' % (cid, worst))
    assert not failures, failures


def fit_params():
    """(cell, placement): every well-posed placement of a cell in one test, except for the lowpass
    3D block kernel at NT 8, where the oracle's lowpass of a window of ~60 features costs it about a
    second per fit -- there one test per placement."""
    out = []
    for cid, cell in E.CELLS.items():
        if not (cell.family == 'lowpass' and cell.ndim == 3 and cell.nt == 8):
            out.append((cid, None))
            continue
        ax = E.AXES[-cell.ndim:]
        out += [(cid, n) for n in ['%s-%s' % (s, a) for a in ax for s in ('low', 'high')] + ['corner-low', 'corner-high']]
    return out


@pytest.mark.parametrize('cid,only', fit_params(), ids=lambda v: v or 'all')
def test_well_posed_clipped_fit_engine_vs_oracle(engine, oracle, cid, only):
    cell = E.CELLS[cid]
    n = 0
    for pl in E.placements(cid):
        if not pl.well_posed or (only and pl.name.split('#')[0] != only):
            continue
        prep, b = pl.free(compute_error=True)
        _, ref = pl.free(compute_error=True)
        engine.refine_batch(prep.problem, b)
        oracle.run_batch(prep.problem, ref)
        assert_engine_matches_oracle(b, ref, cell.ndim, std_from_oracle(cell), pl.id)
        n += 1
    assert n >= (1 if only else 2 * cell.ndim + 2)   # the faces and the corners at least
