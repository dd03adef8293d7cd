"""The kernel cells of the engine's dispatch and one deterministic case per cell.

``ctr_plan_create`` (clustertracking_amd/csrc/ctrefine.hip) sends every cluster to one template
instantiation; ``ctr_cluster_kernel`` (include/ctrefine.h) reports which.  A *cell* is one such
instantiation as the dispatch reaches it, one non-null entry of the handle's kernel table
(``ctr_handle::kernels``, indexed by family, ndim, iso and slot; filled by ``kernel_of`` from
tu_small.hip, the tu_block*.hip units through block_table.h, and tu_large.hip).
``launchable_cells()`` writes them out from what those units instantiate, not from the function
under test.  ``TOO_LARGE_CELLS`` lists the clusters the engine refuses (status 5).

``build_case(cell)`` draws, with a fixed seed, a frame per cluster holding one compact patch of
touching features (``artificial.draw_feature`` with the cell's profile, low Poisson noise) and a
start table whose clusters land in the cell.  For the block kernels the clusters sit at both
edges of the cell's tile band, nv = 16 (NT - 1) and nv = 16 NT - 1 (nv optimiser variables,
NT = ceil((nv + 1) / 16)); ``param_mode`` (cluster / var / const per column) and the number of
features are chosen to hit each edge.  Where an edge cannot be reached the nearest reachable nv
is taken and ``Case.notes`` says why.
"""
import collections
import itertools

import numpy as np
import pandas as pd

import clustertracking_amd as cta
from clustertracking_amd import _abi, artificial
from clustertracking_amd import constraints as cons

MAXF = 64     # features per cluster of the small / block kernels (engine_dims.h)
MAXNT = 8     # tiles of 16 columns of the block kernel (engine_dims.h)
GEOMS = ((2, True), (2, False), (3, True), (3, False))
PROFILES = ('gauss', 'ring', 'disc', 'inv_series')
INV_ORDER = 2                     # inv_series_2 fits every geometry (CTR_MAX_PARAMS)
NOISE_SIZE = {2: 1.0, 3: (0.5, 1.0, 1.0)}
SEED = 20261015

Cell = collections.namedtuple('Cell', 'family ndim iso kind nt lanes')
# family: 'small', 'gauss', 'gauss_tp' (CTR_FLAG_THROUGHPUT table), 'lowpass', 'ring', 'disc',
#         'inv_series', 'large', 'large_lowpass'
# kind:   'small1', 'small2', 'block', 'cons' (constrained instantiation), 'large'
FAMILY_CODE = {'small': _abi.KFAM_SMALL, 'gauss': _abi.KFAM_GAUSS, 'gauss_tp': _abi.KFAM_GAUSS_TP,
               'lowpass': _abi.KFAM_LOWPASS, 'ring': _abi.KFAM_RING, 'disc': _abi.KFAM_DISC,
               'inv_series': _abi.KFAM_INV_SERIES, 'large': _abi.KFAM_LARGE,
               'large_lowpass': _abi.KFAM_LARGE_LOWPASS}
KIND_CODE = {'small1': _abi.KBIN_SMALL1, 'small2': _abi.KBIN_SMALL2, 'block': _abi.KBIN_BLOCK,
             'cons': _abi.KBIN_CONS, 'large': _abi.KBIN_LARGE}


def cell_id(c):
    g = '%dd-%s' % (c.ndim, 'iso' if c.iso else 'aniso')
    if c.kind in ('small1', 'small2'):
        return '%s-%s-%s-%dlanes' % (c.family, g, 'single' if c.kind == 'small1' else 'pair', c.lanes)
    if c.kind == 'large':
        return '%s-%s' % (c.family, g)
    return '%s-%s-%s%d' % (c.family, g, 'cons' if c.kind == 'cons' else 'nt', c.nt)


def launchable_cells():
    cells = []
    for nd, iso in GEOMS:
        # tu_small.hip: singles at 8 / 64 lanes, pairs at 64 / 16 lanes (one table slot each)
        for kind, lanes in (('small1', 8), ('small1', 64), ('small2', 64), ('small2', 16)):
            cells.append(Cell('small', nd, iso, kind, 0, lanes))
        # block kernels (block_table.h): NT 1..8 and the constrained NT 1..2 of every family; the
        # CTR_FLAG_THROUGHPUT family of the gaussian in 2D only (its 3D cells stay null)
        for fam in ('gauss', 'gauss_tp', 'lowpass', 'ring', 'disc', 'inv_series'):
            if fam == 'gauss_tp' and nd == 3:
                continue
            for nt in range(1, MAXNT + 1):
                cells.append(Cell(fam, nd, iso, 'block', nt, 0))
            for nt in (1, 2):
                cells.append(Cell(fam, nd, iso, 'cons', nt, 0))
        # tu_large.hip: without / with the lowpass
        for fam in ('large', 'large_lowpass'):
            cells.append(Cell(fam, nd, iso, 'large', 0, 0))
    return cells


# Clusters beyond the engine (CTR_STATUS_TOO_LARGE): (id, why, profile, geometry, how to reach)
# The case holds the refused cluster and, in the same call, an ordinary one (`companion` features).
TooLarge = collections.namedtuple('TooLarge', 'name why profile ndim iso spec')
TOO_LARGE_CELLS = (
    # (only 3D anisotropic profiles have enough columns: 4 x 8 + 1 = 33 variables)
    TooLarge('cons-ring-3d-aniso', 'constrained cluster over 31 variables (a profile with every column free)',
             'ring', 3, False, dict(constraint='tetramer', n=4, companion=2,
                                    modes=dict(size='var', thickness='var'))),
    TooLarge('cons-disc-3d-aniso', 'constrained cluster over 31 variables (a profile with every column free)',
             'disc', 3, False, dict(constraint='tetramer', n=4, companion=3,
                                    modes=dict(size='var', disc_size='var'))),
    TooLarge('large-inv_series-2d-aniso', 'over 64 features with a profile other than gauss',
             'inv_series', 2, False, dict(n=MAXF + 1, companion=5, modes={})),
    TooLarge('large-gauss-2d-iso-no-per-feature-var', 'large-cluster path without a per-feature variable',
             'gauss', 2, True, dict(n=20, companion=1, modes=dict(signal='cluster', pos='cluster'))),
)


# ---- feature geometry per (ndim, profile) -------------------------------------------------------

def geometry(profile, ndim, iso, wide=False):
    """(size per axis, diameter per axis, profile kwargs of draw_feature, profile columns)."""
    if profile == 'gauss':
        size = {(2, True): (2., 2.), (2, False): (2.5, 2.), (3, True): (1.5,) * 3,
                (3, False): (1.5, 2., 2.)}[(ndim, iso)]
    else:
        size = {(2, True): (3., 3.), (2, False): (3.5, 3.), (3, True): (2.5,) * 3,
                (3, False): (2.5, 3., 3.)}[(ndim, iso)]
    diam = tuple(int(4 * s) + 1 for s in size)
    if profile == 'gauss' and ndim == 3:   # windows of <= 600 px: the 8-lane singles
        diam = (7, 7, 7) if iso else (7, 9, 9)
    if wide:   # windows over 600 px: the 64-lane singles
        diam = {(2, True): (27, 27), (2, False): (27, 25), (3, True): (11,) * 3, (3, False): (11, 13, 13)}[(ndim, iso)]
    extra = dict(gauss=({}, {}), ring=(dict(thickness=0.3), dict(thickness=0.3)),
                 disc=(dict(disc_size=0.5), dict(disc_size=0.5)),
                 inv_series=(dict(p=(1., 1.3, 0.75)), dict(signal_mult=1., param_a=1.3, param_b=0.75)))[profile]
    return size, diam, extra[0], extra[1]


def fit_function(profile):
    return 'inv_series_%d' % INV_ORDER if profile == 'inv_series' else profile


def _columns(profile, ndim, iso):
    ff = cta.fitfunc.FitFunctions(fit_function(profile), ndim, iso)
    return ff


def _lattice(n, ndim, pitch):
    """n points of a cubic lattice of the given pitch, nearest the centre first (a compact patch)."""
    side = int(np.ceil(n ** (1. / ndim))) + 1
    g = np.stack([a.ravel() for a in np.meshgrid(*[np.arange(side)] * ndim, indexing='ij')], 1).astype(float)
    c = (side - 1) / 2.
    d = np.sum((g - c) ** 2, 1) + 1e-6 * np.arange(len(g))   # (a fixed order among ties)
    pts = g[np.argsort(d, kind='stable')[:n]] * np.asarray(pitch)
    return pts - pts.mean(0)


def _shape(ndim, diam, n, pitch):
    ext = np.ceil((int(np.ceil(n ** (1. / ndim))) + 1) * np.asarray(pitch) + 2 * np.asarray(diam) + 4)
    return tuple(int(e) for e in ext)


UNIT_SHAPES = {
    'dimer': lambda nd: np.array([[0.] * nd, [0.] * (nd - 1) + [1.]]),
    'trimer': lambda nd: np.array([[0.] * nd, [0.] * (nd - 1) + [1.],
                                   [0.] * (nd - 2) + [np.sqrt(3) / 2, 0.5]]),
    'tetramer': lambda nd: np.array([[0., 0.], [0., 1.], [1., 0.], [1., 1.]]) if nd == 2 else
    np.array([[1., 1., 1.], [1., -1., -1.], [-1., 1., -1.], [-1., -1., 1.]]) / (2 * np.sqrt(2)),
}
CONS_OF_N = {2: 'dimer', 3: 'trimer', 4: 'tetramer'}


# ---- parameter modes --------------------------------------------------------------------------

def _mode_options(profile, ndim, iso):
    """Candidate param_mode dicts, most ordinary first: (param_mode, n_per_feature, n_shared,
    preference).  Positions are always free per feature."""
    ff = _columns(profile, ndim, iso)
    extras = ff.params[2 + ndim + (1 if iso else ndim):]
    fitted_extras = [e for e in extras if e != 'signal_mult']   # (signal_mult duplicates signal)
    out = []
    ext_opts = [('const', 'cluster', 'var')] * len(fitted_extras)
    for bg, sig, size in itertools.product(('cluster', 'const'), ('var', 'cluster', 'const'),
                                           ('const', 'cluster', 'var')):
        for ex in itertools.product(*ext_opts):
            mode = dict(background=bg, signal=sig, size=size)
            mode.update(zip(fitted_extras, ex))
            ncol_size = 1 if iso else ndim
            npf = ndim + (sig == 'var') + ncol_size * (size == 'var') + sum(e == 'var' for e in ex)
            nsh = (bg == 'cluster') + (sig == 'cluster') + ncol_size * (size == 'cluster') + \
                sum(e == 'cluster' for e in ex)
            # preference: the defaults, and for the other profiles their own parameters fitted
            pref = (bg != 'cluster') + (sig != 'var') + (size != 'const')
            pref += sum(e != 'cluster' for e in ex) if profile != 'gauss' else 0
            out.append((mode, npf, nsh, pref))
    return out


def _n_vars(npf, nsh, n):
    return npf * n + nsh


def _nt(nv):
    return (nv + 1 + 15) // 16


def _plan_block(profile, ndim, iso, nt, target, n_choices, default_small):
    """(param_mode, n, nv) for a cluster of the block kernel with NT = nt, nv nearest `target`."""
    best = None
    for mode, npf, nsh, pref in _mode_options(profile, ndim, iso):
        is_default = pref == 0 and profile == 'gauss'
        for n in n_choices:
            if n > min(16 * nt, MAXF):
                continue
            if default_small and is_default and n <= 2:
                continue              # (the small kernel's)
            nv = _n_vars(npf, nsh, n)
            if _nt(nv) != nt or nv < 1:
                continue
            key = (abs(nv - target), pref, -n)
            if best is None or key < best[0]:
                best = (key, mode, n, nv)
    assert best is not None, (profile, ndim, iso, nt, target)
    return best[1], best[2], best[3]


# ---- cases ------------------------------------------------------------------------------------

class Cluster(object):
    def __init__(self, n, mode, nv=None, constraint=None, note=None, spread=None):
        self.n, self.mode, self.nv, self.constraint, self.note = n, mode, nv, constraint, note
        self.spread = spread


class Case(object):
    """One cell's frames, start table and refine options; ``prepare()`` -> PreparedBatch."""

    def __init__(self, cell, profile, ndim, iso, clusters, flags=0, lowpass=False, wide=False,
                 notes=()):
        self.cell, self.profile, self.ndim, self.iso = cell, profile, ndim, iso
        self.clusters, self.flags, self.lowpass, self.wide = clusters, flags, lowpass, wide
        self.notes = list(notes)
        self.mode = clusters[0].mode
        kinds = set(c.constraint for c in clusters) - {None}
        assert all(c.mode == self.mode for c in clusters) and len(kinds) <= 1
        self.constraint = kinds.pop() if kinds else None   # (one constraint kind per call)
        self.size, self.diameter, self.draw_kw, self.extra_val = geometry(profile, ndim, iso, wide)
        self._draw()

    @property
    def n_features(self):
        return [c.n for c in self.clusters]

    def _draw(self):
        nd = self.ndim
        rng = np.random.RandomState(SEED + 7919 * hash_cell(self.cell))
        pitch = 0.7 * np.asarray(self.diameter, float)   # touching: inside the separation
        shape = _shape(nd, self.diameter, MAXF + 1, pitch)   # (one shape per geometry: cases merge)
        signal = 150. if self.profile != 'inv_series' else 120.
        frames, rows = [], []
        ff = _columns(self.profile, nd, self.iso)
        for k, cl in enumerate(self.clusters):
            if cl.constraint is not None:
                pts = UNIT_SHAPES[cl.constraint](nd) * pitch
                pts = pts - pts.mean(0)
            elif cl.spread is not None:
                pts = np.zeros((cl.n, nd))
                pts[1, -1] = cl.spread     # a pair this far apart (px, last axis)
                pts -= pts.mean(0)
            else:
                pts = _lattice(cl.n, nd, pitch)
            jitter = rng.uniform(-0.3, 0.3, pts.shape)
            if cl.spread is not None:
                jitter[:] = jitter[0]         # (the pair keeps its distance, starts included)
            truth = pts + (np.asarray(shape) - 1) / 2. + jitter
            im = np.zeros(shape, np.uint8)
            for p in truth:
                artificial.draw_feature(im, p, self.size, signal, self.profile, **self.draw_kw)
            im = artificial.add_poisson_noise(im, 2, rng)
            frames.append(im)
            p0 = truth + rng.uniform(-0.25, 0.25, truth.shape)
            if cl.spread is not None:
                p0 = truth + p0[0] - truth[0]
            t = pd.DataFrame(p0, columns=['z', 'y', 'x'][-nd:])
            t['frame'] = k
            t['signal'] = signal * 0.95
            t['background'] = 2.
            sizes = ff.size_columns
            for col, s in zip(sizes, self.size if not self.iso else self.size[:1]):
                t[col] = s * 1.03
            for col, v in self.extra_val.items():
                t[col] = v if col == 'signal_mult' else v * 1.04
            rows.append(t)
        self.frames = np.stack(frames)
        self.f0 = pd.concat(rows, ignore_index=True)

    def kwargs(self):
        kw = dict(fit_function=fit_function(self.profile), param_mode=dict(self.mode))
        if self.constraint is not None:
            dist = 0.7 * np.asarray(self.diameter, float)
            kw['constraints'] = getattr(cons, self.constraint)(tuple(dist), self.ndim)
        if self.lowpass:
            kw['noise_size'] = NOISE_SIZE[self.ndim]
        return kw

    def prepare(self, compute_error=True):
        prep = cta.prepare_batch(self.f0.copy(), cta.ArrayReader(self.frames), self.diameter,
                                 compute_error=compute_error, **self.kwargs())
        prep.problem.flags |= self.flags
        return prep


def hash_cell(cell):
    key = cell_id(cell) if isinstance(cell, Cell) else cell.name
    return sum((i + 1) * ord(ch) for i, ch in enumerate(key))


def _edges(nt):
    return 16 * (nt - 1), 16 * nt - 1


def build_case(cell):
    """The cases of one launchable cell (a list; see the module docstring)."""
    nd, iso = cell.ndim, cell.iso
    if cell.kind == 'small1':
        wide = cell.lanes == 64
        return [Case(cell, 'gauss', nd, iso, [Cluster(1, {}, ndim_nv(nd, iso, 1)) for _ in range(3)], wide=wide)]
    if cell.kind == 'small2':
        size, diam, _, _ = geometry('gauss', nd, iso)
        close = 0.22 * min(d // 2 for d in diam)     # < a quarter of the mask radius
        far = 0.6 * min(diam)
        if cell.lanes == 64:
            cls = [Cluster(2, {}, spread=far), Cluster(2, {}, spread=far * 0.8), Cluster(2, {}, spread=close)]
            return [Case(cell, 'gauss', nd, iso, cls)]
        # CTR_FLAG_THROUGHPUT, >= 64 pairs: the close ones at 64 lanes, the others at 16
        cls = [Cluster(2, {}, spread=close if k % 8 == 0 else far * (0.75 + 0.05 * (k % 5))) for k in range(64)]
        return [Case(cell, 'gauss', nd, iso, cls, flags=_abi.FLAG_THROUGHPUT)]
    fam = cell.family
    profile = fam if fam in ('ring', 'disc', 'inv_series') else 'gauss'
    lowpass = fam in ('lowpass', 'large_lowpass')
    flags = _abi.FLAG_THROUGHPUT if fam == 'gauss_tp' else 0
    notes = []
    if cell.kind == 'large':
        # past MAXF features; past 127 variables with at most MAXF features (sizes free: one
        # param_mode per call, so a case of its own)
        mode, n, nv = _plan_block_large(nd, iso)
        return [Case(cell, profile, nd, iso, [Cluster(MAXF + 1, {}, ndim_nv(nd, iso, MAXF + 1))],
                     flags=flags, lowpass=lowpass),
                Case(cell, profile, nd, iso, [Cluster(n, mode, nv)], flags=flags, lowpass=lowpass,
                     notes=[] if nv == 128 else ['nv = 128 unreachable: %d' % nv])]
    lo, hi = _edges(cell.nt)
    n_choices = (2, 3, 4) if cell.kind == 'cons' else range(1, MAXF + 1)
    out = []
    for target in (lo, hi):
        mode, n, nv = _plan_block(profile, nd, iso, cell.nt, target, n_choices,
                                  cell.kind != 'cons' and not lowpass)
        if nv == target:
            note = None
        elif cell.kind == 'cons':
            note = 'nv = %d unreachable with 2..4 constrained features: %d' % (target, nv)
        elif target == 0:
            note = 'nv = 0 is no fit: %d' % nv
        else:
            note = 'nv = %d unreachable with at most %d features: %d' % (target, MAXF, nv)
        out.append(Case(cell, profile, nd, iso,
                        [Cluster(n, mode, nv, constraint=CONS_OF_N[n] if cell.kind == 'cons' else None)],
                        flags=flags, lowpass=lowpass, notes=[note] if note else []))
    return out


def _npf_nsh(profile, nd, iso, mode):
    for m, npf, nsh, _ in _mode_options(profile, nd, iso):
        if m == mode:
            return npf, nsh
    raise KeyError(mode)


def ndim_nv(nd, iso, n):
    """nv of the default modes (signal and positions per feature, background per cluster)."""
    return (nd + 1) * n + 1


def _plan_block_large(nd, iso):
    """The default modes reach nv = 128 only where (nd + 1) n + 1 = 128; else sizes free."""
    if (128 - 1) % (nd + 1) == 0:
        return {}, 127 // (nd + 1), 128
    best = None
    for mode, npf, nsh, pref in _mode_options('gauss', nd, iso):
        for n in range(1, MAXF + 1):
            nv = _n_vars(npf, nsh, n)
            if nv >= 128 and (best is None or (nv, pref) < best[0]):
                best = ((nv, pref), mode, n, nv)
    return best[1], best[2], best[3]


def build_too_large(tl):
    """A case of one TOO_LARGE_CELLS entry: the refused cluster first, then its companion."""
    sp = tl.spec
    cls = [Cluster(sp['n'], sp['modes'], constraint=sp.get('constraint')), Cluster(sp['companion'], sp['modes'])]
    return Case(tl, tl.profile, tl.ndim, tl.iso, cls)


# ---- one call per problem type ------------------------------------------------------------------

ProblemType = collections.namedtuple('ProblemType', 'name ndim iso family')
TYPE_MODE = {'ring': dict(thickness='cluster'), 'disc': dict(disc_size='cluster'),
             'inv_series': dict(param_a='cluster', param_b='cluster')}


def problem_types():
    return [ProblemType('%dd-%s-%s' % (nd, 'iso' if iso else 'aniso', fam), nd, iso, fam)
            for nd, iso in GEOMS
            for fam in ('gauss', 'gauss_tp', 'lowpass', 'ring', 'disc', 'inv_series')
            if not (fam == 'gauss_tp' and nd == 3)]


def build_type_case(t):
    """One call holding a cluster of every cell one problem type reaches with ONE param_mode: the
    block kernel at NT 1..8 (the upper edge of each band, nv = 16 NT - 1, or the nearest below),
    a constrained cluster, and for the gaussian tables the singles, the pairs (64 of them, some
    close, with CTR_FLAG_THROUGHPUT: both tiers) and a cluster of MAXF + 1 features."""
    profile = t.family if t.family in ('ring', 'disc', 'inv_series') else 'gauss'
    mode = dict(background='cluster', signal='var', size='const', **TYPE_MODE.get(t.family, {}))
    npf, nsh = _npf_nsh(profile, t.ndim, t.iso, mode)
    gauss_default = profile == 'gauss' and t.family != 'lowpass'
    ns = []
    for nt in range(1, MAXNT + 1):
        n = (16 * nt - 1 - nsh) // npf
        assert _nt(_n_vars(npf, nsh, n)) == nt and (n > 2 or not gauss_default)
        ns.append(n)
    kind = next(k for k in ('trimer', 'tetramer') if {'trimer': 3, 'tetramer': 4}[k] not in ns)
    cls = [Cluster(n, mode, _n_vars(npf, nsh, n)) for n in ns]
    m = {'trimer': 3, 'tetramer': 4}[kind]
    cls.append(Cluster(m, mode, _n_vars(npf, nsh, m), constraint=kind))
    if gauss_default:
        _, diam, _, _ = geometry('gauss', t.ndim, t.iso)
        close, far = 0.22 * min(d // 2 for d in diam), 0.6 * min(diam)
        cls += [Cluster(1, mode) for _ in range(3)]
        cls += [Cluster(2, mode, spread=close if k % 8 == 0 else far * (0.75 + 0.05 * (k % 5)))
                for k in range(64 if t.family == 'gauss_tp' else 8)]
    if t.family in ('gauss', 'lowpass'):
        cls.append(Cluster(MAXF + 1, mode))
    return Case(t, profile, t.ndim, t.iso, cls, lowpass=t.family == 'lowpass',
                flags=_abi.FLAG_THROUGHPUT if t.family == 'gauss_tp' else 0)


def all_cases():
    """{cell id: [Case, ...]} for every launchable cell."""
    out = {}
    for c in launchable_cells():
        out[cell_id(c)] = build_case(c)
    return out
