"""The kernel cells of the dispatch and their cases (tests/_dispatch.py), without a GPU.

Every launchable template instantiation has a case; ``ctr_cluster_kernel`` -- the decision
``ctr_plan_create`` takes -- places each case's clusters in the intended cell; ``prepare_batch``
finds the intended clusters; and the C oracle fits every case, so that a disagreement in
tests/test_gpu_dispatch_matrix.py points at the engine, not at a bad case."""
import collections
import itertools

import numpy as np
import pytest
from numpy.testing import assert_equal

import _dispatch as D
from clustertracking_amd import _abi, _lib
from clustertracking_amd.utils import validate_tuple as cta_tuple

CELLS = D.launchable_cells()
FAMILIES = sorted(set(c.family for c in CELLS))


@pytest.fixture(scope='module')
def cases():
    return D.all_cases()


def test_cell_list():
    ids = [D.cell_id(c) for c in CELLS]
    assert len(set(ids)) == len(ids)
    per_family = collections.Counter(c.family for c in CELLS)
    # per geometry (2D/3D x iso/aniso): 4 small tiers; NT 1..8 + constrained 1..2 per block table
    # (the throughput table in 2D only); large without / with lowpass
    assert per_family == {'small': 16, 'gauss': 40, 'gauss_tp': 20, 'lowpass': 40, 'ring': 40,
                          'disc': 40, 'inv_series': 40, 'large': 4, 'large_lowpass': 4}
    assert len(CELLS) == 244


def _problem_sweep():
    """(problem, n) over every parameter-mode choice, profile, lowpass, flag and constraint."""
    for nd, iso in D.GEOMS:
        for profile in D.PROFILES:
            for lowpass, flags, kind in itertools.product((False, True), (0, _abi.FLAG_THROUGHPUT),
                                                          (None, 'dimer', 'trimer', 'tetramer')):
                if lowpass and profile != 'gauss':
                    continue          # (rejected: CTR_ERR_UNSUPPORTED)
                for wide in (False, True):
                    _, diam, _, _ = D.geometry(profile, nd, iso, wide)
                    ff = D._columns(profile, nd, iso)
                    for mode, _, _, _ in D._mode_options(profile, nd, iso):
                        ff2 = type(ff)(D.fit_function(profile), nd, iso, mode)
                        p = _abi.make_problem(nd, iso, ff2.modes, [d // 2 for d in diam],
                                              None if kind is None else (kind, [5.] * nd),
                                              noise_size=cta_tuple(D.NOISE_SIZE[nd], nd) if lowpass else None,
                                              fit_function=D.fit_function(profile))
                        p.flags |= flags
                        yield p, range(1, D.MAXF + 3)


def test_no_launchable_cell_is_missing():
    """Whatever ctr_cluster_kernel answers over a sweep of problems is a listed cell (or status 5),
    lane width included, and every listed cell is answered somewhere in the sweep -- except the
    16-lane pairs: that tier is chosen on the device per batch (front_load_kernel), the host
    function reports a pair's 64 lanes; its case is checked against the device rule in
    test_every_cell_has_cases_in_its_cell."""
    listed = {(D.FAMILY_CODE[c.family], D.KIND_CODE[c.kind], c.nt, c.lanes, c.ndim, c.iso) for c in CELLS}
    device_tier = {(D.FAMILY_CODE[c.family], D.KIND_CODE[c.kind], c.nt, c.lanes, c.ndim, c.iso)
                   for c in CELLS if c.kind == 'small2' and c.lanes == 16}
    seen = set()
    for p, ns in _problem_sweep():
        for n in ns:
            k = _lib.cluster_kernel(p, n)
            assert k.n_vars == _lib.load().ctr_cluster_n_vars(p, n)
            if k.bin == _abi.KBIN_TOO_LARGE:
                assert k.family == _abi.KFAM_NONE
                continue
            key = (k.family, k.bin, k.nt, k.lanes, p.ndim, bool(p.isotropic))
            assert key in listed and key not in device_tier, key
            seen.add(key)
    assert seen == listed - device_tier and len(device_tier) == 4


def test_cluster_kernel_rejects_bad_input():
    p = _abi.make_problem(2, True, [3, 1, 1, 1, 0], (4, 4))
    with pytest.raises(ValueError):
        _lib.cluster_kernel(p, -1)
    p.ndim = 4
    with pytest.raises(ValueError):
        _lib.cluster_kernel(p, 1)


def _small_pair_tiers(prep):
    """(close, far) pair counts by front_load_kernel's rule: starts closer than a quarter of the
    mask radius (scaled per axis)."""
    b, nd = prep.batch, prep.problem.ndim
    r = np.array([prep.problem.radius[a] for a in range(nd)], float)
    d = (b.params[b.feat_offset[:-1], 2:2 + nd] - b.params[b.feat_offset[:-1] + 1, 2:2 + nd]) / r
    close = np.sum(d * d, 1) < 0.0625
    return int(close.sum()), int((~close).sum())


@pytest.mark.parametrize('family', FAMILIES)
def test_every_cell_has_cases_in_its_cell(cases, family):
    for cell in CELLS:
        if cell.family != family:
            continue
        cs = cases[D.cell_id(cell)]
        assert cs, D.cell_id(cell)
        nvs = []
        for case in cs:
            prep = case.prepare()
            n = np.diff(prep.batch.feat_offset)
            assert_equal(n, case.n_features)          # prepare_batch finds the intended clusters
            assert prep.batch.n_clusters == len(case.clusters)
            for cl, m in zip(case.clusters, n):
                k = _lib.cluster_kernel(prep.problem, int(m))
                assert (k.bin, k.family, k.nt) == (D.KIND_CODE[cell.kind], D.FAMILY_CODE[cell.family],
                                                   cell.nt), D.cell_id(cell)
                if cl.nv is not None:
                    assert k.n_vars == cl.nv
                nvs.append(k.n_vars)
                if cell.kind == 'small1':
                    assert k.lanes == cell.lanes
            if cell.kind == 'small2':
                close, far = _small_pair_tiers(prep)
                vol = np.prod([2 * prep.problem.radius[a] + 1 for a in range(cell.ndim)])
                if cell.lanes == 16:
                    # both tiers launch: CTR_FLAG_THROUGHPUT, >= 64 pairs, windows <= 600 px
                    assert prep.problem.flags & _abi.FLAG_THROUGHPUT
                    assert prep.batch.n_clusters >= 64 and vol <= 600 and close > 0 and far > 0
                else:
                    assert close > 0 and far > 0
        if cell.kind in ('block', 'cons'):
            # both edges of the tile band, or the nearest reachable nv with the reason recorded
            lo, hi = 16 * (cell.nt - 1), 16 * cell.nt - 1
            for edge in (lo, hi):
                if edge not in nvs:
                    assert any(n for c in cs for n in c.notes if 'nv = %d' % edge in n), (D.cell_id(cell), edge)
        if cell.kind == 'large':
            assert any(n > D.MAXF for c in cs for n in c.n_features)
            assert any(n <= D.MAXF and v > 127 for c in cs for n, v in zip(c.n_features, [cl.nv for cl in c.clusters]))


def test_tile_band_edges_reached():
    """Every unconstrained block cell reaches both edges of its band, nv = 16 (NT - 1) and
    16 NT - 1, except nv = 0 (no variable: no fit)."""
    for cell in CELLS:
        if cell.kind != 'block':
            continue
        nvs = [cl.nv for c in D.build_case(cell) for cl in c.clusters]
        edges = [e for e in (16 * (cell.nt - 1), 16 * cell.nt - 1) if e > 0]
        assert all(e in nvs for e in edges), (D.cell_id(cell), nvs)


@pytest.mark.parametrize('tl', D.TOO_LARGE_CELLS, ids=lambda t: t.name)
def test_too_large_cells(tl):
    prep = D.build_too_large(tl).prepare()
    n = np.diff(prep.batch.feat_offset)
    assert_equal(n, [tl.spec['n'], tl.spec['companion']])
    assert _lib.cluster_kernel(prep.problem, int(n[0])).bin == _abi.KBIN_TOO_LARGE
    assert _lib.cluster_kernel(prep.problem, int(n[1])).bin == _abi.KBIN_BLOCK


@pytest.mark.parametrize('family', FAMILIES)
def test_oracle_fits_every_case(cases, oracle, family):
    """The C oracle converges (status 0) on every case of the family."""
    for cell in CELLS:
        if cell.family != family:
            continue
        for case in cases[D.cell_id(cell)]:
            prep = case.prepare()
            oracle.run_batch(prep.problem, prep.batch)
            assert (prep.batch.status == 0).all(), (D.cell_id(cell), prep.batch.status)
            assert np.isfinite(prep.batch.cost).all()


def test_oracle_fits_companions_of_too_large(oracle):
    for tl in D.TOO_LARGE_CELLS:
        prep = D.build_too_large(tl).prepare()
        oracle.run_batch(prep.problem, prep.batch)
        assert prep.batch.status[1] == 0, tl.name
