"""The small kernels of aux_kernels.h at exact ties and value edges (tests/_aux_edges.py).  Needs
a real MI355X.

Cluster labelling: ``find.label_frames_device`` against ``find.label_frames`` (cKDTree, the
reference's rule) -- equal order, same partition, equal sizes, the id the smallest row of the
cluster -- on features at a scaled distance of exactly 1, one ulp next to it, at distance 0, and on
frames whose population sits on the edges of the kernel's 256-thread stride.
Frame maximum: ``engine.frame_max_device`` against ``arr.reshape(n, -1).max(1).astype(float64)``,
bit for bit where that is a number and NaN exactly where that is NaN.
Result rows: ``ctr_batch.result_rows`` of a batch of unequal clusters, a refused one among them."""
import numpy as np
import pytest
from numpy.testing import assert_equal

import _aux_edges as A
import _dispatch as D
import clustertracking_amd as cta
from clustertracking_amd import _abi, find

pytestmark = pytest.mark.gpu


# ---- A. cluster labelling --------------------------------------------------------------------------

def same_partition(a, b):
    fa, fb = {}, {}
    for x, y in zip(np.asarray(a), np.asarray(b)):
        if fa.setdefault(x, y) != y or fb.setdefault(y, x) != x:
            return False
    return True


def assert_labels_equal_reference(pos, frames, sep, what):
    sep = np.asarray(sep, dtype=np.float64)
    o_ref, ids, sizes = find.label_frames(pos, frames, sep)
    o_dev, ids_d, sizes_d = find.label_frames_device(pos, frames, sep)
    assert_equal(o_dev, o_ref, err_msg=what)
    wrong = np.flatnonzero(sizes_d != sizes)
    detail = [(int(frames[o_ref][r]), pos[o_ref][frames[o_ref] == frames[o_ref][r]].tolist(), int(sizes[r]),
               int(sizes_d[r])) for r in wrong[:6]]
    assert len(wrong) == 0, '%s: %d rows of %d with another cluster size; (frame, features, reference, ' \
        'device): %s' % (what, len(wrong), len(sizes), detail)
    assert same_partition(ids, ids_d), what
    assert (ids_d <= np.arange(len(ids_d))).all(), what
    assert (ids_d[ids_d] == ids_d).all(), what
    assert_equal(ids_d, A.canonical_ids(ids), err_msg=what)     # the smallest row of the cluster
    return ids, sizes


@pytest.mark.parametrize('sep', A.TIE_SEPARATIONS, ids=str)
def test_find_clusters_exact_ties_follow_the_reference_rule(engine, sep):
    """Every tie, near-tie, duplicate and triple configuration of one separation, each in a frame
    of its own, in one call."""
    configs = A.tie_configs(sep)
    pos, frames = A.assemble(configs)
    ids, sizes = assert_labels_equal_reference(pos, frames, sep, 'separation %s' % (sep,))
    # (what the reference says about them: duplicates are one cluster, a triple 3, 1 + 2 or 1 + 1 + 1)
    by_frame = dict(zip(frames[np.argsort(frames, kind='stable')], sizes))
    for k, c in enumerate(configs):
        if c.kind == 'dup' and len(c.pts) < 3:
            assert by_frame[k] == len(c.pts)


@pytest.mark.parametrize('ndim', (2, 3))
def test_find_clusters_frame_populations_at_the_thread_stride(engine, ndim):
    """0, 1, 255, 256, 257 and 513 features, empty frames between full ones, a permuted chain of
    300, two frames with the same features: through ``label_frames_device`` (which never hands
    an empty frame on) and through ``Engine.find_clusters`` with the empty frames in the table."""
    pos, offset, sep = A.population_case(ndim)
    counts = np.diff(offset)
    frames = np.repeat(np.arange(len(counts)), counts)
    perm = np.random.RandomState(3).permutation(len(pos))
    assert_labels_equal_reference(pos[perm], frames[perm], sep, '%dD, shuffled rows' % ndim)
    ids, sizes = assert_labels_equal_reference(pos, frames, sep, '%dD' % ndim)
    labels, sizes_d = engine.find_clusters(pos, offset, sep)
    assert_equal(sizes_d, sizes)
    assert_equal(labels, A.canonical_ids(ids))
    a, b = slice(offset[8], offset[9]), slice(offset[9], offset[10])     # the coincident frames
    assert_equal(labels[b] - offset[9], labels[a] - offset[8])
    assert labels[b].min() >= offset[9]
    # a table of nothing but empty frames, and one feature behind empty frames
    lab, siz = engine.find_clusters(np.zeros((0, ndim)), np.zeros(4, np.int32), sep)
    assert len(lab) == 0 and len(siz) == 0
    lab, siz = engine.find_clusters(np.ones((1, ndim)), np.array([0, 0, 0, 1], np.int32), sep)
    assert lab.tolist() == [0] and siz.tolist() == [1]


# ---- B. frame maximum ------------------------------------------------------------------------------

def device_frame_max(engine, case):
    import torch
    dtype = case.buf.dtype
    host = case.buf.view(np.int16) if dtype == np.uint16 else case.buf
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    out = torch.full((case.n_frames,), -7., dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    engine.frame_max_device(t.data_ptr() + case.offset * dtype.itemsize, _abi.DTYPE_CODES[dtype], case.n_frames,
                            case.frame_elems, out.data_ptr())
    engine.synchronize()
    return out.cpu().numpy()


def assert_frame_max(engine, cases):
    n = 0
    for case in cases:
        got, exp = device_frame_max(engine, case), A.fm_expected(case)
        assert_equal(np.isnan(got), np.isnan(exp), err_msg='%s: got %s, NumPy %s' % (case.name, got, exp))
        num = ~np.isnan(exp)
        assert_equal(got[num].view(np.uint64), exp[num].view(np.uint64),
                     err_msg='%s: got %s, NumPy %s' % (case.name, got, exp))
        n += 1
    return n


@pytest.mark.parametrize('dtype', A.FM_DTYPES, ids=lambda d: np.dtype(d).name)
def test_frame_max_finds_the_maximum_at_every_loop_and_chunk_edge(engine, dtype):
    assert assert_frame_max(engine, A.fm_placement_cases(dtype)) > 100


@pytest.mark.parametrize('dtype', A.FM_DTYPES, ids=lambda d: np.dtype(d).name)
def test_frame_max_at_the_ends_of_the_pixel_range(engine, dtype):
    assert assert_frame_max(engine, A.fm_value_cases(dtype)) >= 6


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_frame_max_is_nan_for_a_nan_of_either_sign(engine, dtype):
    """NumPy's max propagates NaN whatever its sign bit (0 * inf has it set); the frames around the
    one with the NaN keep their maximum."""
    assert assert_frame_max(engine, A.fm_nan_cases(dtype)) > 200


def test_refine_gives_the_same_for_a_nan_pixel_of_either_sign(engine, oracle):
    """A NaN pixel outside every mask makes the norm, and with it every cost, NaN
    (refine.py:354): the same for both sign bits, as in the C oracle."""
    a, b, f0, diameter = A.nan_twin_frames()
    runs = []
    for im in (a, b):
        prep = cta.prepare_batch(f0.copy(), im, diameter)
        ref = _abi.HostBatch(prep.batch.frames, prep.batch.frame_index, prep.batch.feat_offset, prep.batch.params,
                             prep.batch.low, prep.batch.high)
        engine.refine_batch(prep.problem, prep.batch)
        oracle.run_batch(prep.problem, ref)
        assert_equal(prep.batch.status, ref.status)
        assert_equal(np.isnan(prep.batch.cost), np.isnan(ref.cost))
        assert np.isnan(ref.cost).all()
        runs.append(prep.batch)
    assert_equal(runs[0].params, runs[1].params)
    for name in ('status', 'cost', 'params_out', 'n_rounds', 'n_iter'):
        assert_equal(getattr(runs[0], name), getattr(runs[1], name), err_msg=name)


# ---- C. result rows of unequal clusters, a refused one among them ------------------------------------

def mixed_batch():
    """Clusters of 1, 2, 9, 64 and 70 features (the singles, pairs, block and large kernels of the
    2D gaussian) and one of 70 features on six pixels of a line, each with more overlapping
    neighbours than the large kernel keeps (CTR_MAX_NEIGHBOURS): status 5."""
    import pandas as pd
    kind = D.ProblemType('aux-mixed', 2, True, 'gauss')
    case = D.Case(kind, 'gauss', 2, True, [D.Cluster(n, {}) for n in (1, 2, 9, 64, 70)])
    k = len(case.frames)
    crowd = pd.DataFrame(dict(y=np.full(70, 42.), x=np.linspace(40., 46., 70)))
    crowd['frame'] = k
    for col in ('signal', 'background', 'size'):
        crowd[col] = case.f0[col].iloc[0]
    case.frames = np.concatenate([case.frames, np.ones((1,) + case.frames.shape[1:], np.uint8)])
    case.f0 = pd.concat([case.f0, crowd], ignore_index=True)
    return case.prepare(compute_error=True), k


def marked_batch():
    """A cluster the plan refuses (mark_kernel) in front of an ordinary one."""
    tl = next(t for t in D.TOO_LARGE_CELLS if t.name == 'large-gauss-2d-iso-no-per-feature-var')
    return D.build_too_large(tl).prepare(compute_error=True), 0


@pytest.mark.parametrize('build', (mixed_batch, marked_batch), ids=lambda f: f.__name__)
def test_result_rows_of_unequal_clusters_and_a_refused_one(engine, build):
    import torch
    from clustertracking_amd.device import DeviceBatch
    prep, refused_frame = build()
    hb = prep.batch
    sizes = np.diff(hb.feat_offset)
    refused = int(np.flatnonzero(hb.frame_index == refused_frame)[0])
    if build is mixed_batch:
        assert sorted(sizes.tolist()) == [1, 2, 9, 64, 70, 70] and sizes[refused] == 70
    assert hb.params_std is not None
    n, pad = hb.n_features, 7
    db = DeviceBatch(prep.problem, hb, device=0, engine=engine, result_rows=n + pad)
    db.run()
    torch.cuda.synchronize()
    rows = db.t['result_rows'].cpu().numpy()
    db.download()
    assert hb.status[refused] == _abi.STATUS_TOO_LARGE
    assert_equal(np.delete(hb.status, refused), 0)
    assert np.isfinite(np.delete(hb.cost, refused)).all()
    assert_equal(rows[:n, :-1], hb.params_out)
    assert_equal(rows[:n, -1], np.repeat(hb.cost, sizes))            # (NaN equals NaN here)
    r = slice(hb.feat_offset[refused], hb.feat_offset[refused + 1])
    assert_equal(rows[r, :-1], hb.params[r])
    assert np.isnan(rows[r, -1]).all() and np.isnan(hb.cost[refused])
    assert np.isnan(hb.params_std[r]).all()
    assert_equal(rows[n:], 0.)
    assert rows.shape == (n + pad, hb.params.shape[1] + 1)
