"""Every launch-decision cell of preprocess, locate, characterize and link (tests/_frontplan.py)
on the MI355X, each against the yardstick of its stage's own file and to that file's strictness:
the helpers are imported from there, not restated.  tests/test_frontplan_cells.py shows without a
GPU that every case lands in its cell and that the yardsticks meet their own caps on it."""
import numpy as np
import pytest

import _characterize
import _frontplan as P
import _locate
import _preprocess
import test_gpu_characterize as TC
import test_gpu_link as TL
import test_gpu_locate as TLOC
import test_gpu_preprocess as TP
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib, find
from clustertracking_amd import link as lk

pytestmark = pytest.mark.gpu

preprocessing = cta.preprocessing


# ---- preprocess -------------------------------------------------------------------------------

def _small_call_works():
    frames = TP._u16_batch(10, 2)
    np.testing.assert_array_equal(cta.bandpass(frames[0], 1, 9), _preprocess.bandpass(frames[0], 1, 9))


@pytest.mark.parametrize('cell', P.cells('preprocess'), ids=P.cell_id)
def test_preprocess_cell(cell, engine):
    """integer frames: images, scale factors, bandpass and lowpass equal the yardstick bit for bit;
    float frames: lowpass equal, the rest inside _check_band / _scale_rtol / _check_u8; both
    scaling strategies byte-equal; a ``ty1`` cell: the next box raises and a call after it works"""
    case = P.build_case(cell)
    plan = P.in_cell(case)
    frames, noise, smooth = case.frames, case.noise, case.smooth
    label = P.cell_id(cell)
    print(label, frames.shape, frames.dtype, 'noise', noise, 'smooth', smooth, plan)
    if case.mode == 'scale':
        images, scales = preprocessing.preprocess_arrays(frames)
        assert images.dtype == np.uint8
        for t, raw in enumerate(frames):
            expect, scale = _preprocess.preprocess(raw)
            assert scales[t] == scale, t
            np.testing.assert_array_equal(images[t], expect)
        return
    lows = preprocessing.lowpass_arrays(frames, noise)
    assert lows.dtype == np.float64
    for t, raw in enumerate(frames):
        np.testing.assert_array_equal(lows[t], _preprocess.lowpass(raw, noise))
    if case.mode == 'lowpass':
        return
    bands = preprocessing.bandpass_arrays(frames, noise, smooth)
    plane = preprocessing.preprocess_arrays(frames, noise, smooth, _strategy=_abi.PRE_BAND_PLANE)
    twice = preprocessing.preprocess_arrays(frames, noise, smooth, _strategy=_abi.PRE_TWICE)
    images, scales = preprocessing.preprocess_arrays(frames, noise, smooth)
    for other in (plane, twice):
        assert other[0].tobytes() == images.tobytes() and other[1].tobytes() == scales.tobytes()
    is_int = TP._is_int(frames)
    assert images.dtype == (frames.dtype if is_int else np.uint8) and bands.dtype == np.float64
    for t, raw in enumerate(frames):
        expect, scale = _preprocess.preprocess(raw, noise, smooth)
        assert np.isfinite(scale)
        if is_int:
            assert scales[t] == scale, t
            np.testing.assert_array_equal(images[t], expect)
            np.testing.assert_array_equal(bands[t], _preprocess.bandpass(raw, noise, smooth))
        else:
            bound, band_max = TP._check_band(bands[t], raw, noise, smooth, None, '%s frame %d:' % (label, t))
            np.testing.assert_allclose(scales[t], scale, rtol=TP._scale_rtol(bound, band_max), atol=0)
            TP._check_u8(images[t], raw, noise, smooth, None, '%s frame %d:' % (label, t))
    if case.next_smooth is not None:
        for call in (preprocessing.bandpass_arrays, preprocessing.preprocess_arrays):
            with pytest.raises(_lib.EngineError):
                call(frames, noise, case.next_smooth)
            _small_call_works()
            assert preprocessing.bandpass_arrays(frames[:1], noise, smooth).tobytes() == bands[:1].tobytes()


# ---- locate -----------------------------------------------------------------------------------

@pytest.mark.parametrize('cell', P.cells('locate'), ids=P.cell_id)
def test_locate_cell(cell, engine):
    """positions, their order and type, and the thresholds equal _locate.compose and
    find.percentile_threshold frame by frame, ``precise`` both ways; a ``ty1`` cell: the next
    box raises and a call after it works"""
    case = P.build_case(cell)
    plan = P.in_cell(case)
    frames, sep, pct = case.frames, case.separation, case.percentile
    ndim = frames.ndim - 1
    print(P.cell_id(cell), frames.shape, frames.dtype, 'separation', sep, 'percentile', pct, plan)
    rows = 0
    for precise in case.precise:
        pos, off, thr = find.locate_arrays(frames, sep, percentile=pct, margin=case.margin, precise=precise)
        assert pos.dtype == np.int32 and pos.shape[1] == ndim and off.dtype == np.int64 and off[0] == 0
        assert off[-1] == len(pos) and thr.dtype == np.float64
        for t in range(len(frames)):
            expect = _locate.compose(frames[t], sep, pct, margin=case.margin, precise=precise)
            got = pos[off[t]:off[t + 1]].astype(np.int64)
            if len(expect) == 0:
                assert len(got) == 0, (precise, t)
            else:
                TLOC._same(got, expect)
            ref_thr = np.float64(find.percentile_threshold(frames[t], pct))
            assert thr[t].tobytes() == ref_thr.tobytes() or (np.isnan(thr[t]) and np.isnan(ref_thr)), (precise, t)
            rows += len(expect)
    print(P.cell_id(cell), 'rows compared:', rows)
    assert rows > 0
    if case.next_separation is not None:
        with pytest.raises(_lib.EngineError):
            find.locate_arrays(frames, case.next_separation, percentile=pct, margin=case.margin)
        again, off2, _ = find.locate_arrays(frames[:1], sep, percentile=pct, margin=case.margin, precise=case.precise[-1])
        assert again.tobytes() == pos[:off[1]].tobytes()


# ---- characterize -----------------------------------------------------------------------------

@pytest.mark.parametrize('cell', P.cells('characterize'), ids=P.cell_id)
def test_characterize_cell(cell, engine):
    """mass and signal exact, size as tests/test_gpu_characterize.py has it (_compare); int32
    positions give what the same positions give as float64, bit for bit"""
    case = P.build_case(cell)
    plan = P.in_cell(case)
    frames, pos, offset, radius, iso = case.frames, case.pos, case.offset, case.radius, case.isotropic
    print(P.cell_id(cell), frames.shape, frames.dtype, 'features', len(pos), 'per frame', np.diff(offset), plan)
    mass, signal, size = find.characterize_arrays(frames, pos, offset, radius, iso)
    assert mass.shape == (len(pos),) and size.shape == ((len(pos),) if iso else (len(pos), 2))
    keys = _characterize.size_keys(2, iso)
    for t in range(len(frames)):
        rows = slice(offset[t], offset[t + 1])
        got = dict(mass=mass[rows], signal=signal[rows])
        for a, k in enumerate(keys):
            got[k] = size[rows] if iso else size[rows, a]
        distinct = (offset[t + 1] - offset[t]) // case.repeat
        once = _characterize.compose(pos[rows][:distinct], frames[t], radius, iso)
        expect = {k: np.tile(v, case.repeat) for k, v in once.items()}      # the table repeats its rows
        TC._compare(got, expect, frames.dtype, radius, iso, 2)
    whole = np.round(pos)
    ref = find.characterize_arrays(frames, whole, offset, radius, iso)
    got = find.characterize_arrays(frames, whole.astype(np.int32), offset, radius, iso)
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()


# ---- link -------------------------------------------------------------------------------------

def _sparse_call_works():
    sparse = TL._levels(TL.Z, 'sparse2d')
    got = lk.link_levels(sparse, tuple(TL.Z['sparse2d_sr']), 0, engine='device')
    np.testing.assert_array_equal(np.concatenate(got), TL.Z['sparse2d_ids'])


@pytest.mark.parametrize('cell', P.cells('link'), ids=P.cell_id)
def test_link_cell(cell, engine):
    """ids identical to the host linker's (assert_same_ids names the level, both link counts and
    both sum d^2 on a mismatch); 31 sources: SubnetOversizeException on both sides; 65
    destinations: EngineError naming the level and 65; a call that works after each refusal"""
    case = P.build_case(cell)
    nets, plan = P.in_cell(case)
    levels, sr, memory = case.levels, case.sr, case.memory
    print(P.cell_id(cell), [len(l) for l in levels], 'largest', max(nets, key=sum), plan)
    status = cell.want['status']
    if status == 1:
        with pytest.raises(lk.SubnetOversizeException):
            lk.link_levels(levels, sr, memory)
        with pytest.raises(lk.SubnetOversizeException) as info:
            lk.link_levels(levels, sr, memory, engine='device')
        assert 'Subnetwork contains 31' in str(info.value)
        _sparse_call_works()
        return
    want = lk.link_levels(levels, sr, memory)
    if status == 2:
        with pytest.raises(_lib.EngineError) as info:
            lk.link_levels(levels, sr, memory, engine='device')
        assert 'level %d' % (2 if memory else 1) in str(info.value) and '65' in str(info.value)
        _sparse_call_works()
        return
    got = lk.link_levels(levels, sr, memory, engine='device')
    TL.assert_same_ids(levels, sr, memory, got, want)
    assert all(g.dtype == np.int64 for g in got)
