"""Every grid-stride kernel of the table stages beyond its first trip (``stage_common.h``).

The stages launch at most ``STAGE_MAX_GRID = 65 536`` workgroups and stride past them; the tables of the
other test files never get there.  Here every stage runs three times -- with the default cap, with
the cap of the handle lowered to 1 (``Engine.stage_max_grid``: one workgroup walks every item and
uses its LDS again on every trip) and to 3 (several workgroups take uneven numbers of trips) -- on
the smallest tables on which every loop takes three trips or more under cap 3: 7 or more items of a
loop that gives a workgroup an item, more than 768 elements of a loop that gives a thread an element.
Every output of a capped run must have the bytes of the default run (the kernels use integer
atomics alone, and every float sum is taken in an order that the input alone decides), and the
default run must equal the stage's yardstick under the assertion of the stage's own test file,
whose helpers and tables are used here.  Then the real cap, once: tables just past 65 536 items.

The last test of the file asserts that the cap is the default again."""
import functools
import time

import numpy as np
import pytest

import _cluster_tracks
import _drift
import _find_link as F
import _find_link_refine as R
import _msd
import _pair_correlation
import _refine_arrays
import _vanhove
import clustertracking_amd as ct
import test_gpu_cluster_tracks as t_tracks
import test_gpu_msd as t_msd
import test_gpu_pair_correlation as t_pcf
import test_gpu_refine_prepare as t_prepare
from clustertracking_amd import _abi, refine
from clustertracking_amd.fitfunc import FitFunctions

gpu = pytest.mark.gpu

CAPS = (1, 3)
DEFAULT_CAP = 65536
CHUNK = _abi.MSD_CHUNK
DR_TILE = 2048                      # drift_kernels.h: rows of frame t - 1 in one LDS table
PAST = DEFAULT_CAP + 3              # items of the tables of the real cap


# ---- the three runs ------------------------------------------------------------------------------
def _fields(res):
    """name -> ndarray or plain value of a result tuple (tensors come to the host)"""
    names = getattr(res, '_fields', None) or [str(i) for i in range(len(res))]
    out = {}
    for name, v in zip(names, res):
        if hasattr(v, 'cpu'):
            v = v.cpu().numpy()
        out[name] = v
    return out


def assert_same_bytes(got, base, what):
    got, base = _fields(got), _fields(base)
    assert list(got) == list(base)
    for name, b in base.items():
        g = got[name]
        if not isinstance(b, np.ndarray):
            assert g == b, (what, name, g, b)
            continue
        assert g.dtype == b.dtype and g.shape == b.shape, (what, name, g.dtype, g.shape, b.shape)
        if g.tobytes() != b.tobytes():
            width = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
            diff = np.flatnonzero(np.ascontiguousarray(g).reshape(-1).view(width) != np.ascontiguousarray(b).reshape(-1).view(width))
            raise AssertionError((what, name, 'first differing elements', diff[:5].tolist(), 'of', g.size,
                                  g.reshape(-1)[diff[:5]].tolist(), b.reshape(-1)[diff[:5]].tolist()))


def three_runs(engine, call, what):
    """``call()`` with the default cap, then with every lowered cap: the same bytes; returns the default run"""
    base = call()
    for cap in CAPS:
        with engine.stage_max_grid(cap):
            got = call()
        assert_same_bytes(got, base, (what, 'cap', cap))
    return base


# ---- the switch ----------------------------------------------------------------------------------
@gpu
def test_the_switch(engine):
    assert engine.set_stage_max_grid(5) == DEFAULT_CAP
    assert engine.set_stage_max_grid(7) == 5
    assert engine.set_stage_max_grid(-1) == -1 and engine.set_stage_max_grid(DEFAULT_CAP + 1) == -1
    assert engine.set_stage_max_grid(DEFAULT_CAP) == 7            # the refused values changed nothing
    assert engine.set_stage_max_grid(1) == DEFAULT_CAP
    assert engine.set_stage_max_grid(0) == 1                      # 0: the default
    assert engine.set_stage_max_grid(0) == DEFAULT_CAP
    assert engine._lib.ctr_set_stage_max_grid(None, 4) == -1      # a null handle
    with engine.stage_max_grid(3) as inside:
        assert inside is engine and engine.set_stage_max_grid(3) == 3
    assert engine.set_stage_max_grid(0) == DEFAULT_CAP
    with pytest.raises(KeyError):
        with engine.stage_max_grid(1):
            with engine.stage_max_grid(2):                        # nested: each restores what it found
                raise KeyError('inside')
    assert engine.set_stage_max_grid(0) == DEFAULT_CAP
    for bad in (-1, DEFAULT_CAP + 1):
        with pytest.raises(ValueError, match='stage_max_grid'):
            with engine.stage_max_grid(bad):
                pass
        assert engine.set_stage_max_grid(0) == DEFAULT_CAP
    assert 'stage_max_grid' not in dir(ct)


# ---- msd_arrays, emsd_arrays ---------------------------------------------------------------------
SPANS_IDS = [3, 0, 2, 1, 5, 0, 3, 1, 9]


@gpu
def test_msd_of_ids_in_any_order(engine):
    """'spans': ids 0 and 1 are dense in LDS, 2 and 3 are read from the sorted rows.  In this order a
    short dense id follows a long one, a sparse id a dense one and the reverse, and an id without
    rows (5) or beyond n_particles (9) follows either: nine trips of one workgroup under cap 1."""
    import torch
    pos, off, par, mpp, wants = t_msd._table('spans')
    L, P = 24, 7
    want = _msd.msd(pos, off, par, L, mpp, particles=SPANS_IDS, n_particles=P)
    per = wants[L][0]
    for m, p in enumerate(SPANS_IDS):                              # the yardstick of the id, whatever the order
        assert p >= 4 or want.msd[m].tobytes() == per.msd[p].tobytes()
    assert np.isnan(want.msd[[4, 8]]).all() and not np.isnan(want.msd[[0, 1, 2, 3, 5, 6, 7]]).any()
    ids = torch.tensor(SPANS_IDS, dtype=torch.int64, device='cuda:0')
    got = three_runs(engine, lambda: ct.msd_arrays(pos, off, par, L, mpp, particles=ids, n_particles=P), 'spans')
    assert got.status == _abi.MSD_OK
    _msd.assert_equal_bits(got, want, 'spans')


SMALL_IDS = [2, 0, 4, 0, 5, 1, 3, 2]


@gpu
@pytest.mark.parametrize('ndim', [2, 3])
def test_msd_of_a_track_with_a_gap_after_one_without(engine, ndim):
    """'small': id 2 has a row in each of the frames 0 .. 4, id 0 none in frames 2 and 3, id 4 starts a
    frame later.  Behind id 2 (or 4) the flags and positions of its frames are still in LDS where id 0
    has its gap: a frame that is not marked absent again would pair with them."""
    import torch
    pos, off, par, mpp, wants = t_msd._table('small_%dd' % ndim)
    L, P = 5, int(par.max()) + 1
    per = wants[L][0]
    assert per.n[2, 0] == 4 and per.n[0].tolist() == [2, 0, 1, 2, 1] and per.n[4, 0] == 4
    want = _msd.Result(*(x[SMALL_IDS] for x in per))
    ids = torch.tensor(SMALL_IDS, dtype=torch.int64, device='cuda:0')
    got = three_runs(engine, lambda: ct.msd_arrays(pos, off, par, L, mpp, particles=ids, n_particles=P), ('small', ndim))
    _msd.assert_equal_bits(got, want, ('small', ndim))


@gpu
def test_msd_of_963_rows(engine):
    """'lengths', every id: msd_check_kernel and msd_rows_kernel stride over the 963 rows, msd_particle_kernel over 8 ids"""
    pos, off, par, mpp, wants = t_msd._table('lengths')
    assert len(par) == 963 > 3 * 256
    got = three_runs(engine, lambda: ct.msd_arrays(pos, off, par, 70, mpp), 'lengths')
    _msd.assert_equal_bits(got, wants[70][0], 'lengths')
    ens = three_runs(engine, lambda: ct.emsd_arrays(pos, off, par, 70, mpp), 'lengths ensemble')
    _msd.assert_equal_bits(ens, wants[70][1], 'lengths ensemble')


@gpu
def test_emsd_chunk_after_chunk(engine):
    """'two_chunks_plus' at L = 3: three chunks of ids times three groups of lags, nine work items.
    Then the ten chunks at L = 460 (test_gpu_msd.py): about 2 000 (chunk, lag group) items, which one
    workgroup under cap 1 reduces in a row with the parity of its double buffer carried from item
    to item; nine chunks have a kmax of 1 < L; msd_pool_kernel strides over the 460 lags."""
    pos, off, par, mpp, wants = t_msd._table('two_chunks_plus')
    ens = three_runs(engine, lambda: ct.emsd_arrays(pos, off, par, 3, mpp), 'two_chunks_plus')
    _msd.assert_equal_bits(ens, wants[3][1], 'two_chunks_plus')
    pos, off, par, P, L, long_id, want = t_msd._shared_lags()
    assert (P + CHUNK - 1) // CHUNK == 10 and L > 256
    t0 = time.time()
    ens = three_runs(engine, lambda: ct.emsd_arrays(pos, off, par, L, 0.5), 'ten chunks')
    print('three runs of the ten chunks at L = %d: %.2f s' % (L, time.time() - t0))
    _msd.assert_equal_bits(ens, want, 'ten chunks')


# ---- vanhove -------------------------------------------------------------------------------------
VH_LAGS, VH_WIDTH, VH_REACH = [1, 2, 4, 6, 9], 0.25, 12.


@functools.lru_cache(maxsize=None)
def _vanhove_table(ndim):
    """Three chunks of ids with spans of 8, 3 and 6 frames (the last chunk holds one id): lags 1 and 2
    have pairs in every chunk, 4 and 6 exceed the span of the second, 9 that of all.  K * ndim * 2 H =
    5 * ndim * 96 counters: vanhove_clear_kernel strides; 15 (chunk, lag) items; 5 lags to finish."""
    tracks = [list(range(8))] * CHUNK + [[0, 1, 2]] * CHUNK + [list(range(1, 7))]
    pos, off, par = _msd.exact_tracks(30 + ndim, tracks, ndim=ndim, extra=[(2, 5), (3, -1)])
    mpp = 0.5 if ndim == 2 else (0.5, 1., 2.)
    return pos, off, par, mpp, _vanhove.vanhove(pos, off, par, VH_LAGS, VH_WIDTH, VH_REACH, mpp)


@gpu
@pytest.mark.parametrize('ndim', [2, 3])
def test_vanhove(engine, ndim):
    pos, off, par, mpp, want = _vanhove_table(ndim)
    H = want.count.shape[-1] // 2
    assert len(VH_LAGS) * ndim * 2 * H > 3 * 256 and int(par.max()) + 1 == 2 * CHUNK + 1
    assert (want.n[:2] > 2 * CHUNK).all() and (want.n[2:4] > 0).all() and want.n[4] == 0
    got = three_runs(engine, lambda: ct.vanhove_arrays(pos, off, par, VH_LAGS, VH_WIDTH, VH_REACH, mpp), ('vanhove', ndim))
    assert got.status == _abi.VANHOVE_OK
    _vanhove.assert_equal_bits(got, want, ('vanhove', ndim))


# ---- pair_correlation ----------------------------------------------------------------------------
PCF_DR = 0.0625                     # 160 bins up to the cutoff of 10: T * B = 1 120 (frame, bin) cells
PCF_CASES = {'none': 'tile_none', 'interior': 'tile_interior', 'arc': 'tile_arc',
             'groups_all': 'tile_groups_all', 'groups_same': 'tile_groups_same', 'groups_other': 'tile_groups_other'}


@functools.lru_cache(maxsize=None)
def _pcf_case(name):
    """a case of test_gpu_pair_correlation.py on the frames of 0, 1, 2, 255, 256, 257 and 513 rows (7
    frames, 7 work items, of which the last three are of one frame), with 160 bins instead of 20"""
    pos, off, kw = t_pcf.CASES[PCF_CASES[name]]
    kw = dict(kw, dr=PCF_DR)
    return pos, off, kw, _pair_correlation.pair_correlation(pos, off, **kw)


@gpu
@pytest.mark.parametrize('name', sorted(PCF_CASES))
def test_pair_correlation(engine, name):
    pos, off, kw, want = _pcf_case(name)
    assert np.diff(off).tolist() == [0, 1, 2, 255, 256, 257, 513] and want.count.size == 7 * 160 > 3 * 256
    got = three_runs(engine, lambda: ct.pair_correlation_arrays(pos, off, **kw), name)
    assert got.status == _abi.PCF_OK
    t_pcf.compare(got, want, kw['edge'], name)


# ---- drift ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drift_video():
    """Eight frames, positions that are multiples of 1/4: frames 1, 2 and 5 have more rows than the
    LDS table of the frame before holds (DR_TILE), so the table is built twice within frame 2 and
    again for frames 3 and 6; frame 3 is empty and frame 4 comes after it; frame 2 repeats an id of
    frame 1 in both of its tables and has an unlinked row"""
    rng = np.random.RandomState(21)
    big = DR_TILE + 52
    sizes = [3, big, big, 0, 5, big, 7, 4]
    frames = []
    for t, n in enumerate(sizes):
        ids = rng.permutation(big)[:n] if n < big else rng.permutation(big)
        frames.append([(int(p), tuple(rng.randint(0, 4000, 2) / 4.)) for p in ids])
    frames[1][DR_TILE + 10] = (frames[1][7][0], frames[1][DR_TILE + 10][1])       # a repeated id, one row in each table
    frames[2][40] = (frames[2][41][0], frames[2][40][1])                           # ... and on the side of frame t
    frames[2][100] = (-1, frames[2][100][1])
    pos, off, par = _drift.table(frames)
    return pos, off, par, {s: _drift.compute_drift(pos, off, par, s) for s in (1, 3)}


@gpu
@pytest.mark.parametrize('smoothing', [1, 3])
def test_drift(engine, smoothing):
    pos, off, par, wants = _drift_video()
    want = wants[smoothing]
    T = len(off) - 1
    assert T == 8 and len(pos) > 3 * 256 and np.diff(off).max() > DR_TILE and (par < 0).sum() == 1
    assert want.n_pairs[3] == want.n_pairs[4] == 0 and want.n_pairs[2] > DR_TILE and want.n_pairs[6] == 7
    got = three_runs(engine, lambda: ct.compute_drift_arrays(pos, off, par, smoothing=smoothing), ('drift', smoothing))
    assert got.status == _abi.DRIFT_OK
    np.testing.assert_array_equal(got.n_pairs, want.n_pairs)
    err, bound = np.abs(got.drift - want.drift), _drift.bound(want, pos)
    print('smoothing', smoothing, 'max |d drift|', err.max())
    assert (err <= bound).all(), (smoothing, err.max(), bound.max())
    out = three_runs(engine, lambda: (ct.subtract_drift_arrays(pos, off, got.drift),), ('subtract', smoothing))[0]
    assert out.tobytes() == (pos - got.drift[_drift.frame_of(off, len(pos))]).tobytes()


@gpu
@pytest.mark.parametrize('threshold', [1, 3])
def test_filter_stubs(engine, threshold):
    _, _, par, _ = _drift_video()
    P = int(par.max()) + 4
    want = _drift.filter_stubs(par, threshold, P)
    got = three_runs(engine, lambda: ct.filter_stubs_arrays(par, threshold, n_particles=P), ('stubs', threshold))
    np.testing.assert_array_equal(got.particle, want.particle)
    np.testing.assert_array_equal(got.count, want.count)
    dropped = (want.particle < 0) & (par >= 0)
    assert (want.particle >= 0).any() and dropped.any() == (threshold == 3)


# ---- cluster_tracks, track_positions -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tracks_video(cs, ndim):
    """the seeded video of test_gpu_cluster_tracks.py (features dropped, strangers, clusters that touch,
    ids changed mid-track, unlinked rows) with 8 frames of 800 clusters: more than 768 features,
    particles and tracks"""
    off, par, clu, pos = _cluster_tracks.random_video(40 + cs, n_frames=8, n_clusters=800, cluster_size=cs, ndim=ndim, extra=3)
    res = _cluster_tracks.cluster_tracks(off, par, clu, cs, 2)
    return off, par, clu, pos, (res, _cluster_tracks.track_positions(pos, off, par, res.track_of_particle, res.n_tracks, cs))


@gpu
@pytest.mark.parametrize('cs,ndim', [(2, 2), (3, 3)])
def test_cluster_tracks(engine, cs, ndim):
    off, par, clu, pos, want = _tracks_video(cs, ndim)
    assert len(off) - 1 == 8 and len(par) > 3 * 256 and want[0].n_tracks > 3 * 256

    def call():
        got, block = t_tracks.check(off, par, clu, pos, cs, 2, want=want)          # equals the yardstick under every cap
        return (got.track_of_particle, got.n_tracks, got.n_members, got.status, block.pos, block.present)
    base = three_runs(engine, call, ('tracks', cs, ndim))
    present = base[5]
    assert (present == cs).any() and (present != cs).any()


# ---- refine.prepare_arrays and the scatter -------------------------------------------------------
def _scatter(engine, ff, prepared, n_clusters):
    """ctr_refine_prepare_device(CTR_PREPARE_SCATTER) of made-up fit results in grouped order"""
    import torch
    n, n_params = int(prepared.params.shape[0]), ff.n_params
    dev = prepared.params.device
    fit = (torch.arange(n * n_params, dtype=torch.float64, device=dev) * 0.25).reshape(n, n_params)
    fit_std = fit + 0.125
    fit_cost = torch.arange(n_clusters, dtype=torch.float64, device=dev) + 0.5
    feat_offset = prepared.feat_offset.contiguous()
    params_out, std_out = (torch.full((n, n_params), -1., dtype=torch.float64, device=dev) for _ in range(2))
    cost_out = torch.full((n,), -1., dtype=torch.float64, device=dev)
    d = _abi.RefinePrepare()
    d.mode, d.ndim, d.n_params, d.n_features, d.n_clusters = _abi.PREPARE_SCATTER, 2, n_params, n, n_clusters
    d.order, d.feat_offset = prepared.order.data_ptr(), feat_offset.data_ptr()
    d.fit_params, d.fit_cost, d.fit_std = fit.data_ptr(), fit_cost.data_ptr(), fit_std.data_ptr()
    d.params_out, d.cost_out, d.std_out = params_out.data_ptr(), cost_out.data_ptr(), std_out.data_ptr()
    engine.on_current_stream(engine.refine_prepare_device, d, dev=dev)
    torch.cuda.current_stream(dev).synchronize()
    return params_out, cost_out, std_out, fit, fit_cost, fit_std


@gpu
@pytest.mark.parametrize('name', ['tile_edges', 'chain', 'straddle', 'frames_257'])
def test_refine_prepare_and_scatter(engine, name):
    """'tile_edges': frames of 255, 0, 256, 1 and 257 rows, five trips of rp_label_kernel and
    rp_tables_kernel under cap 1, and 769 rows for the loops over the rows; 'frames_257': 257 frames"""
    case = _refine_arrays.cases()[name]
    want = t_prepare._want(name)
    ff = None

    def call():
        nonlocal ff
        ff, got = t_prepare._device(case)
        return got
    got = three_runs(engine, call, name)
    t_prepare._equal(got, want, ff.n_params)
    if case.pos.shape[1] != 2 or not len(want.label):
        return
    c = len(want.frame_index)
    params_out, cost_out, std_out, fit, fit_cost, fit_std = (
        x.cpu().numpy() for x in three_runs(engine, lambda: _scatter(engine, ff, got, c), (name, 'scatter')))
    order = want.order.astype(np.int64)
    cluster_of = np.repeat(np.arange(c), np.diff(want.feat_offset))
    expect_params, expect_std = np.empty_like(fit), np.empty_like(fit)
    expect_cost = np.empty(len(order))
    expect_params[order], expect_std[order], expect_cost[order] = fit, fit_std, fit_cost[cluster_of]
    np.testing.assert_array_equal(params_out, expect_params)
    np.testing.assert_array_equal(std_out, expect_std)
    np.testing.assert_array_equal(cost_out, expect_cost)


@gpu
@pytest.mark.parametrize('name', sorted(_refine_arrays.INFEASIBLE))
def test_refine_prepare_infeasible(engine, name):
    """rp_feasible_kernel takes the smallest offending parameter with an atomicMin across its trips"""
    case = _refine_arrays.cases()[name]
    ff = None

    def call():
        nonlocal ff
        ff, got = t_prepare._device(case)
        return got
    got = three_runs(engine, call, name)
    assert got.status == (_abi.PREPARE_INFEASIBLE, ff.params.index(_refine_arrays.INFEASIBLE[name]))


# ---- find_link(refine=True) ----------------------------------------------------------------------
RANDOM = F.random_cases()[:10]
# dense videos: a level of more rows than one trip of the workgroups of a level refines (16 rows of
# a 2D window of up to 17 x 17 pixels, 4 rows of a 3D window), so that under a lowered cap the
# kernel does stride over it.  Seeds whose yardstick flags no level as coupled: assert_same compares
# no row of a coupled level, and the ids of the levels behind one follow from how it was linked
DENSE = [('dense_2d', F.video((144, 176), 4, 90, 2012, 'uint8'), dict(F.ISO2, minmass=600., memory=1)),
         ('dense_3d', F.video((24, 48, 48), 4, 28, 2009, 'uint16', size=(1.3, 1.7, 1.7), drift=1.),
          dict(F.ANISO3, minmass=300 * 300., memory=1))]
LINKED = [RANDOM[0], RANDOM[4]] + DENSE


@functools.lru_cache(maxsize=None)
def _linked_want(index):
    name, frames, kw = LINKED[index]
    return R.find_link(frames, **kw)


@gpu
@pytest.mark.parametrize('index', range(len(LINKED)), ids=[c[0] for c in LINKED])
def test_find_link_refine(engine, index):
    name, frames, kw = LINKED[index]
    ndim, iso = frames.ndim - 1, F.is_isotropic(kw)
    want = _linked_want(index)
    got = three_runs(engine, lambda: ct.find_link_arrays(frames, refine=True, **kw), name)
    assert not got.status.any()
    if name.startswith('dense'):
        rows = np.diff(got.frame_offset)
        assert rows.min() > (2 * 16 if ndim == 2 else 2 * 4) and not want['coupled'].any(), rows
    R.assert_same(F.from_arrays(got, ndim, iso), want, ndim, iso, exact=frames.dtype.kind in 'ui')
    assert np.any(got.pos != np.rint(got.pos))


# ---- the real cap: tables just past 65 536 items --------------------------------------------------
@gpu
def test_msd_of_more_ids_than_the_grid(engine):
    """'small_2d' with 65 539 reported ids cycling over 0 .. P + 1: the workgroups 0, 1 and 2 of the
    full grid take a second id.  Row m has the bytes of the yardstick's row of id particles[m]."""
    import torch
    pos, off, par, mpp, wants = t_msd._table('small_2d')
    P, L = int(par.max()) + 1, 5
    per_id = _msd.msd(pos, off, par, L, mpp, particles=range(P + 2), n_particles=P + 2)       # once per distinct id
    ids = np.arange(PAST) % (P + 2)
    got = ct.msd_arrays(pos, off, par, L, mpp, particles=torch.from_numpy(ids).cuda(), n_particles=P + 2)
    assert got.msd.shape == (PAST, L) and got.status == _abi.MSD_OK
    want = _msd.Result(per_id.msd[ids], per_id.mean_d[ids], per_id.mean_d2[ids], per_id.n[ids], per_id.max_d[ids])
    _msd.assert_equal_bits(got, want, 'ids past the grid')


PERIOD = 7


def long_table(n_frames):
    """Frames of one or two rows that repeat a period of 7 frames: one is empty (2), one has a repeated
    id (4), ids 0 and 1 come and go.  Positions are multiples of 1/4 in [0, 8)^2: every sum is exact."""
    rng = np.random.RandomState(77)
    ids = [[0, 1], [1, 0], [], [0], [0, 0], [1, 0], [1]]
    one = [[(p, tuple(rng.randint(0, 32, 2) / 4.)) for p in rows] for rows in ids]
    return _drift.table([one[t % PERIOD] for t in range(n_frames)])


def tiled(per_frame, n_frames, first=0):
    """per-frame values of the frames first .. first + 6 of a table of ``long_table`` -> those of n_frames frames"""
    per_frame = np.asarray(per_frame)
    assert len(per_frame) == PERIOD
    return per_frame[(np.arange(n_frames) - first) % PERIOD]


def expected_drift(n_frames):
    """(drift, n_pairs) of ``long_table(n_frames)`` from the yardstick of its first 8 frames: the step
    of a frame depends on the frame and the one before, so frames 1 .. 7 are one period of steps."""
    pos, off, par = long_table(PERIOD + 1)
    head = _drift.compute_drift(pos, off, par, 0)
    dx, n_pairs = tiled(head.dx[1:], n_frames, 1), tiled(head.n_pairs[1:], n_frames, 1)
    dx[0], n_pairs[0] = 0., 0
    return np.cumsum(dx, axis=0), n_pairs          # multiples of 1/8 far below 2^53: the running sum is exact


PCF_LONG = dict(cutoff=4., dr=1., boundary=[[0., 0.], [8., 8.]])


def expected_pcf(n_frames, edge):
    """the yardstick's Result of ``long_table(n_frames)`` from that of one period: a frame's count, weight,
    n_ref, n_rows and g_frame depend on the frame alone (the boundary is given); clause 10 pools the
    denominators frame by frame, in frame order, as the yardstick does"""
    pos, off, _ = long_table(PERIOD)
    one = _pair_correlation.pair_correlation(pos, off, edge=edge, **PCF_LONG)
    count, weight, g_frame = (tiled(x, n_frames) for x in (one.count, one.weight, one.g_frame))
    n_ref, n_rows = tiled(one.n_ref, n_frames), tiled(one.n_rows, n_frames)
    _, _, shell = _pair_correlation.bins(PCF_LONG['cutoff'], PCF_LONG['dr'], 2)
    with np.errstate(invalid='ignore', divide='ignore'):
        rho = (one.n_rows - 1).astype(np.float64) / np.float64(64.)
        den = (rho[:, None] * shell[None, :]) * one.weight
        good = (den > 0) & (den < np.inf)
        total, any_frame = np.zeros(len(shell)), np.zeros(len(shell), dtype=bool)
        for t in range(n_frames):
            ok = good[t % PERIOD]
            total[ok] += den[t % PERIOD][ok]
            any_frame |= ok
        g = np.where(any_frame, count.sum(0) / total, np.nan)
    return _pair_correlation.Result(one.r_edges, g, g_frame, count, weight, n_ref, n_rows)


LONG_SEPARATION, LONG_RADIUS = (3., 3.), (2, 2)


def _long_start_values(pos, ff):
    out = np.tile(np.arange(ff.n_params, dtype=np.float64) + 1., (len(pos), 1))
    for a, col in enumerate(ff.pos_columns):
        out[:, ff.params.index(col)] = pos[:, a]
    return out


def expected_prepare(n_frames, ff):
    """the yardstick's Prepared of ``long_table(n_frames)`` from that of one period: the clusters of a
    frame depend on the frame alone; labels and the order shift by the 9 rows of a period, the
    clusters of a period follow those of the one before"""
    pos, off, _ = long_table(PERIOD)
    one = _refine_arrays.prepare(pos, off, _long_start_values(pos, ff), LONG_SEPARATION, ff, None, LONG_RADIUS)
    n_one, c_one = len(pos), len(one.frame_index)
    full_pos, full_off, _ = long_table(n_frames)
    n, periods = len(full_pos), -(-n_frames // PERIOD)
    c = int(np.searchsorted(one.frame_index, n_frames - (periods - 1) * PERIOD)) + (periods - 1) * c_one

    def rows(x, shift):
        x = np.concatenate([np.asarray(x) + k * shift for k in range(periods)]) if shift else np.tile(x, (periods,) + (1,) * (np.ndim(x) - 1))
        return x
    label, size, order = rows(one.label, n_one)[:n], rows(one.cluster_size, 0)[:n], rows(one.order, n_one)[:n]
    feat_offset = np.append(rows(one.feat_offset[:-1], n_one)[:c], n).astype(np.int32)
    frame_index = rows(one.frame_index, PERIOD)[:c]
    return _refine_arrays.Prepared(label.astype(np.int32), size.astype(np.int32), order.astype(np.int32), feat_offset,
                                   frame_index.astype(np.int32), rows(one.params, 0)[:n], rows(one.low, 0)[:n], rows(one.high, 0)[:n])


def test_the_tiled_expectations_equal_the_yardsticks():
    """No device.  On three periods and a part of a fourth (24 frames) the expectations that the long
    table is compared with are the yardsticks' results on the whole table.  Measured on the whole
    table of 65 539 frames (one core of the host the suite was written on): _drift.compute_drift
    0.8 s, _pair_correlation.pair_correlation 2.0 s for edge 'none' and 10.3 s for 'arc',
    _refine_arrays.prepare 1.3 s, where they gave the arrays of the tiled expectations; those take
    0.6 s together."""
    n_frames = 3 * PERIOD + 3
    pos, off, par = long_table(n_frames)
    assert np.diff(off).tolist() == ([2, 2, 0, 1, 2, 2, 1] * 4)[:n_frames] and set(pos.reshape(-1) * 4 % 1) == {0.}
    want = _drift.compute_drift(pos, off, par, 0)
    drift, n_pairs = expected_drift(n_frames)
    assert drift.tobytes() == want.drift.tobytes() and (n_pairs == want.n_pairs).all() and want.n_pairs.max() == 2
    assert set(want.n_pairs[1:8].tolist()) == {0, 1, 2} and np.abs(want.drift[-1]).max() > 0
    for edge in ('none', 'arc'):
        want = _pair_correlation.pair_correlation(pos, off, edge=edge, **PCF_LONG)
        tile = expected_pcf(n_frames, edge)
        for name in want._fields:
            assert getattr(tile, name).dtype == getattr(want, name).dtype, name
            np.testing.assert_array_equal(getattr(tile, name), getattr(want, name), err_msg=name)
        assert want.count.sum() > 0 and not np.isnan(want.g).all()
    ff = FitFunctions('gauss', 2, True, None)
    want = _refine_arrays.prepare(pos, off, _long_start_values(pos, ff), LONG_SEPARATION, ff, None, LONG_RADIUS)
    tile = expected_prepare(n_frames, ff)
    for name in want._fields:
        assert getattr(tile, name).dtype == getattr(want, name).dtype, name
        np.testing.assert_array_equal(getattr(tile, name), getattr(want, name), err_msg=name)
    assert want.cluster_size.max() == 2 and want.cluster_size.min() == 1


@functools.lru_cache(maxsize=None)
def _long():
    return long_table(PAST)


@gpu
def test_drift_of_more_frames_than_the_grid(engine):
    pos, off, par = _long()
    assert len(off) - 1 == PAST
    drift, n_pairs = expected_drift(PAST)
    got = ct.compute_drift_arrays(pos, off, par)
    assert got.status == _abi.DRIFT_OK
    np.testing.assert_array_equal(got.n_pairs, n_pairs)
    np.testing.assert_array_equal(np.diff(got.drift, axis=0), np.diff(drift, axis=0))      # dx, frame by frame
    assert got.drift.tobytes() == drift.tobytes()


@gpu
@pytest.mark.parametrize('edge', ['none', 'arc'])
def test_pair_correlation_of_more_frames_than_the_grid(engine, edge):
    pos, off, _ = _long()
    want = expected_pcf(PAST, edge)
    got = ct.pair_correlation_arrays(pos, off, edge=edge, **PCF_LONG)
    assert got.status == _abi.PCF_OK and got.g_frame.shape == (PAST, 4)
    t_pcf.compare(got, want, edge, ('long', edge))


@gpu
def test_refine_prepare_of_more_frames_than_the_grid(engine):
    pos, off, _ = _long()
    ff = FitFunctions('gauss', 2, True, None)
    want = expected_prepare(PAST, ff)
    got = refine.prepare_arrays(pos, off, _long_start_values(pos, ff), LONG_SEPARATION, ff, None, LONG_RADIUS)
    t_prepare._equal(got, want, ff.n_params)


# ---- the last test of the file -------------------------------------------------------------------
@gpu
def test_the_cap_is_the_default_again(engine):
    assert engine.set_stage_max_grid(0) == DEFAULT_CAP
