"""The launch-decision cells of preprocess, locate, characterize and link and their cases
(tests/_frontplan.py), without a GPU.

Every cell has a case whose restated plan lands in the cell; every link case has the sub-network
it claims (from the host candidate graph) and, where it must solve, the host linker solves it;
every preprocess float case keeps the yardstick's own at-threshold pixels and ``p_ref`` inside
the caps of tests/test_gpu_preprocess.py -- so that a disagreement in
tests/test_gpu_frontend_matrix.py points at the engine, not at a bad case."""
import collections

import numpy as np
import pytest

import _frontplan as P
import _preprocess
import test_gpu_link as TL
import test_gpu_preprocess as TP
from clustertracking_amd import link as lk

CELLS = P.cells()


def test_cell_list():
    ids = [P.cell_id(c) for c in CELLS]
    assert len(set(ids)) == len(ids)
    per_stage = collections.Counter(c.stage for c in CELLS)
    # preprocess: 9 + 6 ty, 4 gauss, 16 z pairs, 3 hx, 4 widths, 4 scale; locate: 6 tiles, 2 big, 2 narrow,
    # 9 + 6 ty, 3 3D, ring, 2 clip, 3 seams; characterize: 2 x (6 types + 8 counts + empty);
    # link: (15 chains + 5 stars + 3 combs) x 2 memories, 2 x 2 refusals, 2 many, 1 big level
    assert per_stage == {'preprocess': 46, 'locate': 34, 'characterize': 30, 'link': 53}


@pytest.mark.parametrize('cell', [c for c in CELLS if c.stage != 'link'], ids=P.cell_id)
def test_case_lands_in_its_cell(cell):
    case = P.build_case(cell)
    plan = P.in_cell(case)
    print(P.cell_id(cell), plan)
    again = P.build_case(cell)          # seeded from the cell's name: the same inputs every time
    for k, v in case.__dict__.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == getattr(again, k).tobytes()


def test_restated_tile_heights_are_all_reached():
    seen = collections.defaultdict(set)
    for cell in CELLS:
        if cell.stage == 'preprocess' and not cell.name.startswith('scale'):
            case = P.build_case(cell)
            p = P.pre_case_plan(case)
            seen['pre', case.frames.dtype.name].add(p.ty)
            seen['pre-pairs', case.frames.dtype.name].add((p.z_gauss, p.z_box))
        if cell.stage == 'locate':
            case = P.build_case(cell)
            seen['loc%dd' % (case.frames.ndim - 1), case.frames.dtype.name].add(P.loc_case_plan(case).ty)
    for dt in ('uint8', 'uint16', 'float64'):
        assert seen['pre', dt] >= {8, 4, 2, 1}, (dt, seen['pre', dt])
    for dt in ('uint8', 'int16', 'float32', 'float64'):
        assert len(seen['pre-pairs', dt]) == 4
    for dt in ('uint16', 'float32', 'float64'):
        assert seen['loc2d', dt] >= {16, 8, 4, 2, 1}
    assert all(1 in seen['loc2d', np.dtype(d).name] and 1 in seen['pre', np.dtype(d).name] for d in P.DTYPES)
    assert {t for k, v in seen.items() if k[0] == 'loc3d' for t in v} >= {8, 4, 2, 1}


def test_existing_inputs_take_one_side_only():
    """the gap this file closes, on record: the geometries of the stages' own GPU files all plan
    ty = 16 (preprocess) and one word, one histogram block, one chunk per frame (locate)"""
    for shape, noise, smooth in TP.GEOMETRIES + TP.FLOAT_GEOMETRIES:
        for dt in (np.uint8, np.float64):
            assert P.pre_plan(shape[1:], dt, 'preprocess', noise, smooth).ty == 16
    for shape, sep in (((40, 52), 6), ((33, 47), (5, 8)), ((40, 40), 5), ((10, 16, 18), (3, 5, 6))):
        p = P.loc_plan(shape, np.float64, sep)
        assert (p.nwx, p.bpf, p.cpf, p.ty) == (1, 1, 1, 16 if len(shape) == 2 else 8)
    for radius in ((4, 4), (6, 6), (3, 7)):
        assert P.chr_plan(2, radius, 80).lanes == 16
    for radius in ((9, 9), (11, 8)):
        assert P.chr_plan(2, radius, 80).lanes == 64
    assert P.chr_plan(2, (8, 8), 1).vol == 289 and P.chr_plan(2, (8, 9), 1).vol == 323


@pytest.mark.parametrize('cell', [c for c in CELLS if c.stage == 'preprocess' and c.name[-3:] in ('f32', 'f64')
                                  and not c.name.startswith('scale')], ids=P.cell_id)
def test_preprocess_float_cases_meet_the_caps_on_the_yardstick(cell):
    """the caps of tests/test_gpu_preprocess.py (_check_band: at most 1 pixel in 1000, floor 1, at
    the threshold; _check_u8: p_ref < 1e-3), met by the yardstick alone on the chosen frames"""
    case = P.build_case(cell)
    if case.mode == 'lowpass':
        return          # the Gaussian chain is the same operations on both sides: compared equal
    ndim = case.frames.ndim - 1
    for t, raw in enumerate(case.frames):
        bound = TP._band_bound(raw, case.smooth)
        band = _preprocess._gaussian_chain(raw, _preprocess.validate_tuple(case.noise, ndim)) - \
            _preprocess.boxcar(raw, case.smooth)
        unsure = int((np.abs(band - 1 / 255.) <= bound).sum())
        expect, _ = _preprocess.preprocess(raw, case.noise, case.smooth)
        other, _ = _preprocess.preprocess(raw, case.noise, case.smooth, bandpass=_preprocess.bandpass_longdouble)
        p_ref = np.mean(expect != other)
        print('%s frame %d: %d pixels at the threshold of %d, p_ref %.3e' % (P.cell_id(cell), t, unsure, raw.size, p_ref))
        assert unsure <= max(1e-3 * raw.size, 1)
        assert p_ref < 1e-3


LINK_CELLS = [c for c in CELLS if c.stage == 'link']


@pytest.mark.parametrize('cell', LINK_CELLS, ids=P.cell_id)
def test_link_case_has_its_subnetwork_and_the_host_answers(cell):
    case = P.build_case(cell)
    nets, plan = P.in_cell(case)
    print(P.cell_id(cell), 'largest', max(nets, key=sum), plan)
    if cell.want['status'] == 1:
        with pytest.raises(lk.SubnetOversizeException):
            lk.link_levels(case.levels, case.sr, case.memory)
    else:       # must solve on the host (status 2 is the device solver's capacity, not the rule's)
        ids = lk.link_levels(case.levels, case.sr, case.memory)
        assert [len(i) for i in ids] == [len(l) for l in case.levels]
        if 'ns' in cell.want and cell.want['status'] == 0:
            # the chain links: most of the smaller side finds a partner
            a = case.pair + (2 if case.memory else 1)
            linked = np.isin(ids[a], np.concatenate(ids[:a])).sum()
            if 'hubs' not in cell.want and 'comb' not in cell.want:
                assert linked >= min(cell.want['ns'], cell.want['nd']) // 2
            # the sources of the sub-network (the row y = 100) that the host leaves unlinked
            mine = np.abs(case.levels[case.pair][:, 0] - 100.) < 2.5
            assert mine.sum() == cell.want['ns']
            unlinked = int((~np.isin(ids[case.pair][mine], ids[a])).sum())
            taken = P.second_column_taken(cell.want['nd'], unlinked)
            print(P.cell_id(cell), 'unlinked sources', unlinked, 'of', cell.want['ns'], '-> a column beyond 64 is assigned:', taken)
            assert taken == ('hubs' in cell.want or 'comb' in cell.want)
            if 'comb' in cell.want:
                assert unlinked == cell.want['ns'] - cell.want['comb'] - 1


def test_random_walkers_never_reach_the_second_column():
    """the largest ns + nd of every existing RANDOM seed, on record (level pairs as memory 0 sees
    them; a memory adds remembered sources to a level, seeds and steps stay the same): below 65,
    so that no lane of the solver owns a second column with several sources anywhere in
    tests/test_gpu_link.py"""
    best = {}
    for c in TL.RANDOM:
        levels = TL.walkers(*c[:8])
        sr = np.asarray(lk.validate_tuple(c[8], c[3]), float)
        best[c[0]] = TL.largest_subnet_sources(levels, sr, destinations=True)
        assert TL.largest_subnet_sources(levels, sr) == max(
            [s for a, b in zip(levels[:-1], levels[1:]) for s, _ in P.subnets(a, b, sr)] or [0])
    print('largest sub-network (sources, destinations) per RANDOM seed:', best)
    assert max(s + d for s, d in best.values()) < 65
    per_level = {c[0]: max(sum(1 for sd in P.subnets(a, b, np.asarray(lk.validate_tuple(c[8], c[3]), float)) if sd != (1, 1))
                           for a, b in zip(*(lambda l: (l[:-1], l[1:]))(TL.walkers(*c[:8]))))
                 for c in TL.RANDOM if c[0] in (2, 3)}
    print('most non-trivial sub-networks in one level, seeds 2 and 3:', per_level)
    # they do reuse the per-wave LDS (more sub-networks than wavefronts) -- with small ones only
    assert min(per_level.values()) > P.LNK_WAVES


def _maxima(case, t, precise):
    import _locate
    return np.asarray(_locate.compose(case.frames[t], case.separation, case.percentile, margin=case.margin,
                                      precise=precise)).reshape(-1, 2).astype(int)


@pytest.mark.parametrize('cell', [c for c in CELLS if c.stage == 'locate' and 'seam' in c.want], ids=P.cell_id)
def test_locate_seam_cases_put_maxima_on_the_seams(cell):
    """word seam: in the yardstick a candidate on one side of x = 63 | 64 (or 127 | 128) is dropped
    for a maximum on the other side that is closer than the separation, and a pair exactly the
    separation apart stays; batch seam: maxima stay in the last rows of frame t and in the first
    rows of frame t + 1, at neighbouring columns"""
    case = P.build_case(cell)
    if cell.want['seam'] == 'word':
        across = kept_pairs = 0
        for t in range(len(case.frames)):
            cand, kept = _maxima(case, t, False), _maxima(case, t, True)
            keep = set(map(tuple, kept))
            for y, x in cand:
                if (y, x) in keep:
                    continue
                for ky, kx in kept:
                    if (x // 64) != (kx // 64) and (y - ky) ** 2 + (x - kx) ** 2 < case.separation ** 2:
                        across += 1
                        break
            for y, x in kept:
                kept_pairs += ((y, x + 5) in keep) and x // 64 != (x + 5) // 64
        print(P.cell_id(cell), 'dropped across a word seam:', across, 'kept at the separation:', kept_pairs)
        assert across >= 6 and kept_pairs >= 1
    else:
        n = 0
        for t in range(len(case.frames) - 1):
            last, first = _maxima(case, t, True), _maxima(case, t + 1, True)
            last, first = last[last[:, 0] >= 30], first[first[:, 0] <= 1]
            n += sum(1 for _, x in last if np.any(np.abs(first[:, 1] - x) <= 1))
        print(P.cell_id(cell), 'pairs across a frame seam:', n)
        assert n >= 6
