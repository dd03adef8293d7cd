"""The edge-window cases (tests/_edge_windows.py) on the CPU: the C oracle's pinned evaluation
against NumPy's, every case's sensitivity to a mistake in the window code, and the well-posed
clipped fits of the oracle against the reference's minimiser."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _edge_windows as E
import ref_numpy

GAUSS_CELLS = [cid for cid, c in E.CELLS.items() if c.family in E.GAUSS_FAMILIES]
MAX_CLUSTERS = 8    # of a 64-pair batch, for the per-cluster NumPy work (close and far pairs)


def run_pinned(oracle, pl):
    b = pl.pinned()
    oracle.run_batch(pl.prep().problem, b)
    return b


def test_cells_and_placements_cover_the_matrix():
    kinds = {(c.ndim, c.iso, c.family, c.kind, c.nt, c.lanes) for c in E.CELLS.values()}
    for nd, iso in ((2, True), (2, False), (3, True), (3, False)):
        for lanes in (8, 64):
            assert (nd, iso, 'small', 'small1', 0, lanes) in kinds
        for lanes in (64, 16):
            assert (nd, iso, 'small', 'small2', 0, lanes) in kinds
        for fam in ('gauss', 'lowpass', 'ring', 'disc', 'inv_series') + (('gauss_tp',) if nd == 2 else ()):
            for nt in (1, 8):
                assert (nd, iso, fam, 'block', nt, 0) in kinds
            assert (nd, iso, fam, 'cons', 1, 0) in kinds
        assert (nd, iso, 'large', 'large', 0, 0) in kinds and (nd, iso, 'large_lowpass', 'large', 0, 0) in kinds
    names = {p.name for p in E.placements('small-2d-iso-single-8lanes')}
    assert {'inside', 'low-y', 'low-x', 'high-y', 'high-x', 'corner-low', 'corner-high', 'thin-y',
            'thin-x1', 'thin-x2', 'thin-x3', 'beyond-low', 'beyond-high', 'limit-low-kept',
            'limit-low-filtered', 'limit-high-kept', 'limit-high-filtered', 'kept_no_pixel',
            'all_filtered', 'ties0-inside', 'ties0-clipped', 'corner-low-u16', 'corner-low-f32'} <= names


def test_tie_fractions_hold_the_known_ones():
    """r = 5: a pixel at (1.4, 4.8) from the centre; r = 13: integer centres (5-12-13), where the
    plain sum is 1.0000000000000002 and the contracted one 1."""
    f5 = {(round(10 * a), round(10 * b)) for a, b, _, exact in E.tie_fractions([5, 5]) if exact}
    assert f5 & {(6, 2), (4, 8), (6, 8), (4, 2), (2, 6), (8, 4), (8, 6), (2, 4)}
    f13 = {(round(10 * a), round(10 * b)): (d, n) for a, b, d, n in E.tie_fractions([13, 13])}
    assert f13[(0, 0)][0] and f13[(0, 0)][1] > 0
    assert E._ellipse([5, 12], [0., 0.], [13, 13], False) > 1. == E._ellipse([5, 12], [0., 0.], [13, 13], True)


@pytest.mark.parametrize('cid', [c for c in E.CELLS if E.CELLS[c].kind != 'cons'])
def test_every_cell_carries_its_kinds_of_tie(cid):
    """Per unconstrained cell: a tie placement whose plain mask sum is exactly 1 somewhere, and,
    where the search finds one for the cell's radii, a rounding-sensitive one (a pixel that a
    contracted sum or ``rel`` from the other origin classifies differently) and one off the integers
    with an exact sum of 1 (r = 5 on the last two axes: the pixel at (1.4, 4.8) from the centre)."""
    pls = [p for p in E.placements(cid) if 'ties' in p.tags]
    rad = E.radius_of(pls[0].case)
    found = E.tie_fractions(rad)
    assert any('ties_exact' in p.tags for p in pls)
    if any(t[2] for t in found):
        assert any('ties_differs' in p.tags for p in pls)
    off = [t[:2] for t in found if t[3] and t[:2] != (0., 0.)]
    if off:
        assert any(p.tie_fraction in off for p in pls)
    assert any(p.tie_fraction == (0., 0.) for p in pls)
    if tuple(rad[-2:]) == (5, 5):
        placed = {(round(10 * p.tie_fraction[0]), round(10 * p.tie_fraction[1])) for p in pls}
        assert placed & {(6, 2), (4, 8), (6, 8), (4, 2), (2, 6), (8, 4), (8, 6), (2, 4)}
    for p in pls:     # the start positions carry the fractional parts
        pos = p.f0[list(E.AXES[-2:])].values
        assert np.allclose(pos - np.floor(pos + 1e-9), p.tie_fraction, atol=1e-9)


def test_some_cell_has_radius_5_on_the_last_axes():
    assert any(tuple(E.radius_of(E.placements(cid)[0].case)[-2:]) == (5, 5) for cid in E.CELLS)


def test_windows_are_what_the_placements_claim():
    """Widths of exactly 1, 2 and 3 on the last axis; an axis 0 below 2 r + 1; the limit twins at
    the filter's last kept and first dropped value; dtype and odd row lengths."""
    for cid in ('small-2d-iso-single-8lanes', 'small-3d-aniso-pair-64lanes', 'gauss-3d-iso-nt8', 'disc-2d-aniso-cons1'):
        pls = {p.name: p for p in E.placements(cid)}
        rad = E.radius_of(pls['inside'].case)
        for w in (1, 2, 3):
            assert pls['thin-x%d' % w].frames.shape[-1] == w
        thin = next(p for n, p in pls.items() if n.startswith('thin-') and 'x' not in n)
        assert thin.frames.shape[1] < 2 * rad[0] + 1
        for name, want in (('limit-low-kept', -rad[-1]), ('limit-low-filtered', -rad[-1] - 1)):
            assert_array_equal(np.round(pls[name].f0.groupby('frame')['x'].min().values), want)
        w = pls['limit-high-kept'].frames.shape[-1]
        assert_array_equal(np.round(pls['limit-high-kept'].f0.groupby('frame')['x'].max().values), w + rad[-1] - 1)
        assert_array_equal(np.round(pls['limit-high-filtered'].f0.groupby('frame')['x'].max().values), w + rad[-1])
    pls = {p.name: p for p in E.placements('small-2d-iso-single-8lanes')}
    assert pls['corner-low-u16'].prep().batch.frames.dtype == np.uint16
    assert pls['corner-low-f32'].prep().batch.frames.dtype == np.float32
    assert pls['corner-low-u16'].frames.shape[-1] % 2 == 1 and pls['corner-low-f32'].frames.shape[-1] % 2 == 1


def test_mutated_subimage_without_mutation_is_the_reference():
    for cid in ('small-2d-iso-pair-64lanes', 'gauss-3d-aniso-nt1'):
        for pl in E.placements(cid):
            prep = pl.prep()
            for c in range(prep.batch.n_clusters):
                params, frame, nd, radius = E._cluster(prep.problem, prep.batch, c)
                a = ref_numpy.subimage(params[:, 2:2 + nd], frame, radius)
                b = E.mutated_subimage(params[:, 2:2 + nd], frame, radius)
                assert (a is None) == (b is None), pl.id
                if a is not None:
                    for x, y in zip(a, b):
                        assert_array_equal(x, y, err_msg=pl.id)


@pytest.mark.parametrize('cid', GAUSS_CELLS)
def test_oracle_pinned_cost_is_numpys(oracle, cid):
    """With every bound pinned to the start the oracle returns the start after one evaluation, and
    its cost is NumPy's reference objective there to rtol 1e-12 (measured: at most 5e-15)."""
    worst = 0.
    for pl in E.placements(cid):
        b = run_pinned(oracle, pl)
        cost, P, status = E.numpy_yardstick(pl.prep().problem, b)
        assert_array_equal(b.status, status, err_msg=pl.id)
        assert_array_equal(b.params_out, b.params, err_msg=pl.id)
        ok = status == 0
        assert (b.n_rounds[ok] == 1).all() and (b.n_iter[ok] == 1).all(), pl.id
        assert np.isnan(b.cost[~ok]).all(), pl.id
        assert_allclose(b.cost[ok], cost[ok], rtol=1e-12, atol=0, err_msg=pl.id)
        if ok.any():
            worst = max(worst, np.max(np.abs(b.cost[ok] / cost[ok] - 1)))
        if pl.name.startswith(('all_filtered', 'kept_no_pixel')):
            assert (status == 1).all(), pl.id
        if pl.name.startswith(('inside', 'low', 'high', 'corner')):
            assert (status == 0).all(), pl.id
    print('%s: worst relative difference %.1e' % (cid, worst))


@pytest.mark.parametrize('cid', list(E.CELLS))
def test_every_case_is_sensitive(cid):
    """The NumPy cost of every case moves by more than 1e-6 relative under each mistake that can
    reach it: the window shifted by one on some axis (a window of a few pixels can hold equal
    values one pixel further along one of them); the clip dropped where the frame cuts the
    window; ``<`` for ``<=`` where a pixel's mask sum is exactly 1; the filter bound off by one
    where that changes which pixels are fitted.  A case without a window (every cluster status 1
    because no feature passes the filter) has no window code to get wrong."""
    unproven, lt_bitten = [], []
    for pl in E.placements(cid):
        prep = pl.prep()
        problem, batch = prep.problem, prep.batch
        bitten = set()
        todo = range(min(batch.n_clusters, MAX_CLUSTERS))
        base = {}
        for c in todo:
            params, frame, nd, radius = E._cluster(problem, batch, c)
            coords = params[:, 2:2 + nd]
            sub = E.mutated_subimage(coords, frame, radius)
            if sub is None:
                continue
            # (the restatement without a mistake is ref_numpy.subimage: the test above)
            base[c] = E.cost_on(problem, batch, c, sub)
            if base[c][2] == 0:
                # (a window of a few pixels can hold equal values one pixel further on one axis)
                assert any(E.moved(base[c], E.cost_on(problem, batch, c, E.shifted(sub, frame, a)))
                           for a in range(nd)), (pl.id, c, 'shift')
                bitten.add('shift')
            if pl.clipped:
                unclipped = E.mutated_subimage(coords, frame, radius, 'noclip')
                if ((unclipped[1] < 0) | (unclipped[1] >= np.asarray(frame.shape)[:, None])).any():
                    # the unclipped window holds mask pixels beyond the frame
                    assert E.moved(base[c], E.cost_on(problem, batch, c, unclipped)), (pl.id, c, 'noclip')
                    bitten.add('noclip')
            if 'ties' in pl.tags and E.has_exact_tie(problem, batch, c):
                assert E.moved(base[c], E.mutated_cost(problem, batch, c, 'lt')), (pl.id, c, 'lt')
                bitten.add('lt')
            if 'limit' in pl.tags:
                b = E.mutated_subimage(coords, frame, radius, 'filter')
                same = b is not None and (
                    sub[1].shape == b[1].shape and np.array_equal(sub[1], b[1]) and np.array_equal(sub[2], b[2]))
                if not same:   # (the same pixels in the same masks: provably the same cost)
                    assert E.moved(base[c], E.cost_on(problem, batch, c, b)), (pl.id, c, 'filter')
                    bitten.add('filter')
        has_window = any(ref_numpy.window(E._cluster(problem, batch, c)[0][:, 2:2 + problem.ndim],
                                          batch.frames[0].shape, E.radius_of(pl.case)) is not None for c in todo)
        if has_window and not bitten:
            unproven.append(pl.id)
        if 'lt' in bitten:
            lt_bitten.append(pl.name)
    assert not unproven, unproven
    if E.CELLS[cid].kind != 'cons':   # a pixel with a mask sum of exactly 1, interior and clipped
        assert any('inside' in n for n in lt_bitten) and any('clipped' in n for n in lt_bitten), lt_bitten


FIT_CELLS = [cid for cid in GAUSS_CELLS if E.CELLS[cid].kind != 'cons']


def fit_params():
    """(cell, placement) of the SLSQP comparison: every well-posed placement of a cell in one test,
    except where a fit takes the reference's minimiser a second or more (NT 8: 112-127 variables,
    0.5-1.4 s; the large path: 196-261 variables) -- there one test per placement, and of the large
    clusters whose fit takes 3-4 s (measured: 2D anisotropic and 3D, two clusters per placement) both
    corners, one low and one high face."""
    out = []
    for cid in FIT_CELLS:
        cell = E.CELLS[cid]
        if cell.kind != 'large' and cell.nt != 8:
            out.append((cid, None))
            continue
        ax = E.AXES[-cell.ndim:]
        names = ['%s-%s' % (s, a) for a in ax for s in ('low', 'high')] + ['corner-low', 'corner-high']
        if cell.kind == 'large' and (cell.ndim == 3 or not cell.iso):
            names = ['low-x', 'high-%s' % ax[0], 'corner-low', 'corner-high']
        out += [(cid, n) for n in names]
    return out


@pytest.mark.parametrize('cid,only', fit_params(), ids=lambda v: v or 'all')
def test_well_posed_clipped_fits_oracle_vs_slsqp(oracle, cid, only):
    """Faces, corners and thin with every centre inside the frame: the oracle and the reference's
    minimiser (SLSQP at tol 1e-14) both converge to positions within 1e-6 px, in one round -- except
    the pairs closer than a quarter of the mask radius (the close ones of _dispatch), which take both
    minimisers two rounds at a high face: there the round counts are equal."""
    n = 0
    for pl in E.placements(cid):
        if not pl.well_posed or (only and pl.name.split('#')[0] != only):
            continue
        prep, a = pl.free(compute_error=False)
        _, b = pl.free(compute_error=False)
        todo = list(range(min(a.n_clusters, MAX_CLUSTERS)))
        oracle.run_batch(prep.problem, a)
        ref_numpy.run_batch(prep.problem, b, tol=1e-14, maxiter=1000, clusters=todo)
        nd = prep.problem.ndim
        for c in todo:
            rows = slice(a.feat_offset[c], a.feat_offset[c + 1])
            spread = pl.case.clusters[c].spread
            close = spread is not None and spread < 0.25 * min(E.radius_of(pl.case))
            assert a.status[c] == 0 and b.status[c] == 0, (pl.id, c, a.status[c], b.status[c])
            assert a.n_rounds[c] == b.n_rounds[c] and (close or a.n_rounds[c] == 1), (pl.id, c, a.n_rounds[c], b.n_rounds[c])
            d = np.abs(a.params_out[rows, 2:2 + nd] - b.params_out[rows, 2:2 + nd]).max()
            assert d < 1e-6, (pl.id, c, d)
        n += 1
    assert n >= 1
