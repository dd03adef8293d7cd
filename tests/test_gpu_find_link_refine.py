"""``ctr_find_link_refine_device`` / ``find_link(refine=True)`` on the MI355X against the
reference's tables (tests/golden/find_link/find_link_refine_cases.npz) and the yardstick loop
(tests/_find_link_refine.py): integer frames bit for bit, float64 frames to 1e-10 (positions) and
rtol 1e-12 (mass, signal, size)."""
import numpy as np
import pytest

import _find_link as F
import _find_link_refine as R
import _preprocess
import _refine_com as RC
import clustertracking_amd as cta

pytestmark = pytest.mark.gpu

FIXTURES = R.fixtures()
RANDOM = F.random_cases()[:10]
PAIRS = R.pair_cases()


@pytest.mark.parametrize('index', range(len(FIXTURES)), ids=[c[0] for c in FIXTURES])
def test_device_equals_the_reference(engine, index):
    name, frames, kw, want = FIXTURES[index]
    ndim, iso = frames.ndim - 1, F.is_isotropic(kw)
    got = cta.find_link_arrays(frames, refine=True, **kw)
    assert not got.status.any()
    R.assert_equals_fixture(F.from_arrays(got, ndim, iso), want, ndim, iso, frames.dtype.kind in 'ui')


@pytest.mark.parametrize('index', range(len(RANDOM)), ids=[c[0] for c in RANDOM])
def test_seeded_videos(engine, index):
    name, frames, kw = RANDOM[index]
    ndim, iso = frames.ndim - 1, F.is_isotropic(kw)
    want = R.find_link(frames, **kw)
    if frames.dtype.kind == 'f':
        assert RC.min_gap(want['offs']) > 1e-9
    got = cta.find_link_arrays(frames, refine=True, **kw)
    assert not got.status.any()
    R.assert_same(F.from_arrays(got, ndim, iso), want, ndim, iso, exact=frames.dtype.kind in 'ui')
    assert np.any(got.pos != np.rint(got.pos))


def test_seeded_videos_relocate_and_walk():
    """what the comparison above relies on (no device)"""
    n_reloc = n_walked = n_clipped = n_uncoupled = 0
    for name, frames, kw in RANDOM:
        want = R.find_link(frames, **kw)
        n_reloc += int(want['relocated'].sum())
        n_walked += int((want['n_iter'] >= 2).sum())
        n_clipped += int(want['clipped'].sum())
        n_uncoupled += int((~want['coupled']).sum())
    assert n_reloc >= 15 and n_walked >= 10 and n_clipped >= 5 and n_uncoupled >= 40, (n_reloc, n_walked, n_clipped)


@pytest.mark.parametrize('name', sorted(PAIRS))
def test_refinement_decides_the_track(engine, name):
    frames, kw = PAIRS[name]
    with_, without = R.find_link(frames, **kw), F.find_link(frames, **kw)
    got = cta.find_link_arrays(frames, refine=True, **kw)
    R.assert_same(F.from_arrays(got, 2, True), with_, 2, True, exact=True)
    plain = cta.find_link_arrays(frames, refine=False, **kw)
    F.assert_same(F.from_arrays(plain, 2, True), without, 2, True, exact=True)
    assert got.particle.tolist() != plain.particle.tolist()
    assert (got.n_tracks, plain.n_tracks) == ((1, 2) if name == 'only_with' else (2, 1))


def test_refine_false_is_the_call_without_the_keyword(engine):
    for index in (0, 1, 2, 9):
        name, frames, kw = RANDOM[index]
        a = cta.find_link_arrays(frames, **kw)
        b = cta.find_link_arrays(frames, refine=False, **kw)
        for x, y in zip(a[:7], b[:7]):
            assert x.tobytes() == y.tobytes()
        assert a.n_tracks == b.n_tracks and np.array_equal(a.coupled, b.coupled)
        F.assert_same(F.from_arrays(b, frames.ndim - 1, F.is_isotropic(kw)), F.find_link(frames, **kw), frames.ndim - 1,
                      F.is_isotropic(kw), exact=frames.dtype.kind in 'ui')


def test_with_noise_size_the_refinement_reads_the_raw_frames(engine):
    """maxima and relocation look at the preprocessed frames, the refinement at the raw ones: a
    pedestal under the raw video, which the bandpass removes, pulls every raw centre of mass towards
    the centre of its window"""
    name, frames, kw = F.random_cases()[12]
    frames = np.clip(frames.astype(np.int64) + 40, 0, 255).astype(np.uint8)
    # (integer frames: the device's preprocessing equals NumPy's bit for bit)
    proc = np.stack([_preprocess.preprocess(f, 1, F._relocate.as_tuple(kw['separation'], 2))[0] for f in frames])
    want = R.find_link(proc, raw_frames=frames, **kw)
    got = cta.find_link_arrays(frames, noise_size=1, refine=True, **kw)
    R.assert_same(F.from_arrays(got, 2, True), want, 2, True, exact=True)
    on_proc = RC.compose(proc, want['start'], want['frame_offset'], (4, 4))
    assert np.abs(on_proc['pos'] - want['pos']).max() > 0.05 and want['relocated'].any()


def test_dataframe_and_arguments(engine):
    name, frames, kw = RANDOM[6]
    want = R.find_link(frames, max_iterations=3, shift_thresh=0.4, **kw)
    f = cta.find_link(frames, refine=True, max_iterations=3, shift_thresh=0.4, **kw)
    assert list(f.columns) == ['y', 'x', 'frame', 'particle', 'mass', 'signal', 'size', 'relocated']
    got = dict(pos=f[['y', 'x']].values, frame=f['frame'].values, particle=f['particle'].values,
               relocated=f['relocated'].values, mass=f['mass'].values, signal=f['signal'].values, size=f['size'].values,
               coupled=want['coupled'], frame_offset=want['frame_offset'], n_tracks=f.attrs['n_tracks'])
    R.assert_same(got, want, 2, True, exact=True)
    assert want['n_iter'].max() == 3 and f.attrs['coupled_levels'] == int(want['coupled'].sum())
    for bad in (dict(max_iterations=0), dict(max_iterations=101), dict(shift_thresh=0.)):
        with pytest.raises(ValueError):
            cta.find_link_arrays(frames, refine=True, **dict(kw, **bad))
    for bad in (1, 'com', lambda **k: None):
        with pytest.raises(NotImplementedError, match='refine takes True'):
            cta.find_link_arrays(frames, refine=bad, **kw)
    # a diameter of 1 is a radius of 0, which the refinement refuses
    with pytest.raises(ValueError, match='radius'):
        cta.find_link_arrays(frames, refine=True, **dict(kw, diameter=1))
    # the call after the refusals computes
    again = cta.find_link(frames, refine=True, max_iterations=3, shift_thresh=0.4, **kw)
    assert again.equals(f)
