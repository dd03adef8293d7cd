"""How a fit ends other than converged, as inputs: the endings of DESIGN.md ("how a fit ends") and
the edit of a start table or of the problem that selects each one.

Every refine kernel family restates the ending rules in its own code (small_kernel_body.inc,
block_kernel_body.inc, large_kernel.h, tail_kernel.h) and the oracle restates them once more
(oracle/ctr_oracle.c: refine_one, solve).  Here each ending is DECIDED BY THE INPUT, far from any
rounding threshold, so that engine and oracle must agree on status, n_rounds and, where the
table gives a number, n_iter.

Built on tests/_dispatch.py: a cell's case gives one cluster; ``copies`` makes a batch of K
byte-identical copies of it on the same frame (the frames do not grow), and ``apply`` edits one.

Per-cluster endings (``PER_CLUSTER``; one copy each in one call, an unedited copy first and last):

  nonfinite             NaN in the signal of the last feature          status 2, n_iter 0, n_rounds 0
  nonfinite_const       +inf in a column whose mode is const           the same
  outside               every position -1000 on every axis             status 1, n_iter 0, n_rounds 1
  empty_interval        low = high + 1, last-axis position, last feat. status 3, n_iter 0, n_rounds 1
  empty_interval_const  low > high on a const column                   no effect: the unedited bytes
  size_zero             sizes of the last feature 0, size const only   status 3, n_iter 0, n_rounds 1
  bound_active          high of the last-axis position of every        status 0; unconstrained clusters
                        feature = start - 0.6 (truth within 0.25)      end bitwise at the bound
  start_clipped         last feature, last-axis position: a finite     status 0, compared with the oracle
                        high 0.1 above the start, then the start
                        0.4 beyond that high

(start_clipped tightens the bound before it steps over it: the table's own upper bound lies a whole
mask radius from the start, and a start beyond THAT is a fit from a radius away, which is decided
by the iteration and not by the input.  With the bound 0.1 above the drawn start an unconstrained
fit moves at most 0.75 px on that axis and 0.25 px on the others from the mask centre, under
max_shift = 1 whatever the noise: one round.  A constrained cluster may move further;
``build_calls`` raises where a first-round shift of bound_active or start_clipped comes within
``SHIFT_CLEAR`` of max_shift.)

Endings with nonfinite_const / empty_interval_const need a const column and size_zero a const size;
a case without one leaves that copy out (``names`` says which copies a call holds).

Per-call endings (``PER_CALL``; a setting of the problem, on two unedited copies):

  solver_limit  solver_maxiter = 2                      status 3, n_iter 2, n_rounds 1
  rms           max_rms_dev = cost of the fit / 2       status 4; n_iter, n_rounds of the unedited fit
  round_cap     max_shift = 0.05, max_iter = 1          status 0, n_rounds 1
  two_rounds    max_shift = 0.05, max_iter = 10         status 0, n_rounds 2

Every ending with status != 0: cost NaN, params_out the bytes of params, params_std all NaN.

``build_calls`` runs the oracle on all of it and RAISES where an expectation would sit near a
threshold: the first-round shift of round_cap / two_rounds must exceed
2 max_shift and the second-round one stay below max_shift / 2 (a case that fails has its starts
shifted by one of ``NUDGES`` or settled on its fit, it is not dropped); bound_active must fit (status 0).

Not reachable by an input-decided case, and so not here: the ``gain <= CTR_STALL_TOL`` edge, where
engine and oracle differ in the last bits, and the ``mu > 1e30`` exit.
"""
import collections
import copy

import numpy as np

import _dispatch as D
from clustertracking_amd import _abi

PER_CLUSTER = ('nonfinite', 'nonfinite_const', 'outside', 'empty_interval', 'empty_interval_const',
               'size_zero', 'bound_active', 'start_clipped')
PER_CALL = ('solver_limit', 'rms', 'round_cap', 'two_rounds')
# name -> (status, n_iter, n_rounds) of the endings that fail by the input alone
FAILS = {'nonfinite': (_abi.STATUS_NONFINITE, 0, 0),
         'nonfinite_const': (_abi.STATUS_NONFINITE, 0, 0),
         'outside': (_abi.STATUS_OUT_OF_BOUNDS, 0, 1),
         'empty_interval': (_abi.STATUS_NO_CONVERGENCE, 0, 1),
         'size_zero': (_abi.STATUS_NO_CONVERGENCE, 0, 1)}
FITS = ('empty_interval_const', 'bound_active', 'start_clipped')
BOUND_BELOW = 0.6        # bound_active: the bound this far below the start
CLIP_ABOVE, CLIP_BEYOND = 0.1, 0.4    # start_clipped: bound above the drawn start, start beyond the bound
SMALL_SHIFT = 0.05       # max_shift of round_cap and two_rounds
NUDGES = (0., 0.2, -0.2, 0.1, -0.1)   # px on the last axis: the starts of a case are shifted by the first
#                                       of these with which its round shifts are clear of max_shift
SETTLED_OFF = 0.2        # px: see build_calls
SHIFT_CLEAR = 1e-3       # bound_active, start_clipped: a first-round shift this far (relative) from max_shift,
#                          a thousand times the 1e-6 px to which engine and oracle agree
WORKERS = 4             # threads of prefetch (ctypes releases the interpreter lock during an oracle call)
PAIRS_16 = 64            # pairs of a call from which the far ones run 16 lanes each
TABLES = ('params_out', 'cost', 'status', 'n_iter', 'n_rounds', 'params_std')


class Columns(object):
    """the columns of a problem: positions, sizes, const ones"""

    def __init__(self, problem):
        self.nd, self.np = problem.ndim, problem.n_params
        self.modes = [problem.modes[i] for i in range(self.np)]
        self.pos = list(range(2, 2 + self.nd))
        self.sizes = list(range(2 + self.nd, 2 + self.nd + (1 if problem.isotropic else self.nd)))
        self.const = [k for k, m in enumerate(self.modes) if m == _abi.MODE_CONST]
        self.size_const = all(self.modes[k] == _abi.MODE_CONST for k in self.sizes)
        self.constraint = {_abi.CONS_DIMER: 2, _abi.CONS_TRIMER: 3, _abi.CONS_TETRAMER: 4}.get(problem.constraint_kind)

    def applicable(self, name):
        if name in ('nonfinite_const', 'empty_interval_const'):
            return bool(self.const)
        if name == 'size_zero':
            return self.size_const
        return True

    def constrained(self, n_features):
        return self.constraint is not None and n_features == self.constraint


def clone(b):
    """a batch with its own start table and bounds (HostBatch keeps an array it is given) and fresh outputs"""
    return _abi.HostBatch(b.frames, b.frame_index, b.feat_offset, b.params.copy(), b.low.copy(), b.high.copy(),
                          want_std=True)


def copies(b, c, k):
    """k copies of cluster c of batch b, on c's frame"""
    rows = np.tile(np.arange(b.feat_offset[c], b.feat_offset[c + 1]), k)
    n = b.feat_offset[c + 1] - b.feat_offset[c]
    return _abi.HostBatch(b.frames, np.repeat(b.frame_index[c], k), n * np.arange(k + 1), b.params[rows],
                          b.low[rows], b.high[rows], want_std=True)


def rows_of(hb, c):
    return slice(int(hb.feat_offset[c]), int(hb.feat_offset[c + 1]))


def apply(hb, c, name, cols):
    """edit cluster c of hb in place"""
    r = rows_of(hb, c)
    last, x = r.stop - 1, cols.pos[-1]
    if name == 'nonfinite':
        hb.params[last, 1] = np.nan
    elif name == 'nonfinite_const':
        hb.params[last, cols.const[0]] = np.inf
    elif name == 'outside':
        hb.params[r, cols.pos[0]:cols.pos[-1] + 1] = -1000.
    elif name == 'empty_interval':
        hb.low[last, x] = hb.high[last, x] + 1.
    elif name == 'empty_interval_const':
        k = cols.const[-1]
        hb.low[last, k], hb.high[last, k] = hb.params[last, k] + 1., hb.params[last, k] - 1.
    elif name == 'size_zero':
        hb.params[last, cols.sizes[0]:cols.sizes[-1] + 1] = 0.
    elif name == 'bound_active':
        hb.high[r, x] = hb.params[r, x] - BOUND_BELOW
    elif name == 'start_clipped':
        hb.high[last, x] = hb.params[last, x] + CLIP_ABOVE
        hb.params[last, x] = hb.high[last, x] + CLIP_BEYOND
    else:
        raise KeyError(name)


def per_cluster_call(b, c, cols, pad=0):
    """(batch, names): an unedited copy, one copy per applicable ending, `pad` unedited ones, an
    unedited copy; names[k] is the ending of copy k or None"""
    names = [None] + [n for n in PER_CLUSTER if cols.applicable(n)] + [None] * (pad + 1)
    hb = copies(b, c, len(names))
    for k, n in enumerate(names):
        if n is not None:
            apply(hb, k, n, cols)
    return hb, names


def subset(b, order, outputs=False):
    """the clusters `order` of batch b, in that order, as a batch of their own (same frames); with
    `outputs` the results of b go along"""
    order = np.asarray(order, dtype=int)
    rows = np.concatenate([np.arange(b.feat_offset[c], b.feat_offset[c + 1]) for c in order])
    off = np.concatenate([[0], np.cumsum(np.diff(b.feat_offset)[order])])
    hb = _abi.HostBatch(b.frames, b.frame_index[order], off, b.params[rows], b.low[rows], b.high[rows],
                        want_std=True)
    if outputs:
        hb.params_out[:], hb.params_std[:] = b.params_out[rows], b.params_std[rows]
        for name in ('cost', 'status', 'n_iter', 'n_rounds'):
            getattr(hb, name)[:] = getattr(b, name)[order]
    return hb


def is_close(hb, c, problem):
    """two starts of cluster c closer than a quarter of the mask radius (front_load_kernel's rule
    for a likely slow fit): nearly coincident features, an ill-conditioned fit"""
    radius = np.array([problem.radius[a] for a in range(problem.ndim)], dtype=float)
    p = hb.params[rows_of(hb, c), 2:2 + problem.ndim] / radius
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return bool((d2[np.triu_indices(len(p), 1)] < 0.0625).any())


def edit_every_third(b, cols, problem, start=1):
    """(batch, names): a copy of b with clusters start, start + 3, ... edited, cycling through the
    endings that apply.  A close cluster (is_close) takes the next ending that fails or changes
    nothing: bound_active and start_clipped are compared with the oracle to 1e-6 px, which needs a
    well-conditioned fit."""
    hb = clone(b)
    cyc = [n for n in PER_CLUSTER if cols.applicable(n)]
    names = [None] * hb.n_clusters
    j = 0
    for c in range(start, hb.n_clusters, 3):
        while is_close(b, c, problem) and cyc[j % len(cyc)] in ('bound_active', 'start_clipped'):
            j += 1
        names[c] = cyc[j % len(cyc)]
        apply(hb, c, names[c], cols)
        j += 1
    return hb, names


def with_settings(problem, **kw):
    p = copy.copy(problem)     # (a ctypes Structure: a bytewise copy)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def call_problem(problem, name, unedited_cost=None):
    """the problem of a per-call ending"""
    if name == 'solver_limit':
        return with_settings(problem, solver_maxiter=2)
    if name == 'rms':
        return with_settings(problem, max_rms_dev=0.5 * float(unedited_cost))
    if name == 'round_cap':
        return with_settings(problem, max_shift=SMALL_SHIFT, max_iter=1)
    if name == 'two_rounds':
        return with_settings(problem, max_shift=SMALL_SHIFT, max_iter=10)
    raise KeyError(name)


def failed_outputs_ok(hb, c):
    """the three byte conditions of a failed cluster"""
    r = rows_of(hb, c)
    return bool(np.isnan(hb.cost[c]) and np.isnan(hb.params_std[r]).all() and
                hb.params_out[r].tobytes() == hb.params[r].tobytes())


def same_bytes(a, ca, b, cb):
    """cluster ca of batch a and cluster cb of batch b have equal outputs, bit for bit"""
    ra, rb = rows_of(a, ca), rows_of(b, cb)
    return all([a.params_out[ra].tobytes() == b.params_out[rb].tobytes(),
                a.params_std[ra].tobytes() == b.params_std[rb].tobytes(),
                a.cost[ca:ca + 1].tobytes() == b.cost[cb:cb + 1].tobytes(),
                a.status[ca] == b.status[cb], a.n_iter[ca] == b.n_iter[cb], a.n_rounds[ca] == b.n_rounds[cb]])


# ---- the calls of one cell's case and the oracle on them ------------------------------------------

def case_cluster(cell):
    """the cluster of a cell's case that is copied: the 16-lane pairs take a far pair (the close
    ones, every eighth, run at 64 lanes)"""
    return 1 if cell.kind == 'small2' and cell.lanes == 16 else 0


def case_pad(cell):
    """unedited copies that a call of the cell needs beyond its own to reach the cell's kernel"""
    return PAIRS_16 if cell.kind == 'small2' and cell.lanes == 16 else 0


Calls = collections.namedtuple('Calls', 'problem cols per_cluster names alone unedited per_call nudged')
# per_cluster: the batch of per_cluster_call; alone: the unedited copies alone (as many as the call
# holds); unedited: index of the first unedited copy; per_call: {name: (problem, batch)}


def shift_of(out, start, cols):
    d = out[:, cols.pos[0]:cols.pos[-1] + 1] - start[:, cols.pos[0]:cols.pos[-1] + 1]
    return np.sqrt((d ** 2).sum(1))


def round_shifts(oracle, problem, hb, c, cols):
    """(largest first-round shift, largest second-round shift) of a feature, from the oracle with
    max_iter 1 and 2 at max_shift = SMALL_SHIFT"""
    one, two = copies(hb, c, 1), copies(hb, c, 1)
    oracle.run_batch(with_settings(problem, max_shift=SMALL_SHIFT, max_iter=1), one)
    oracle.run_batch(with_settings(problem, max_shift=SMALL_SHIFT, max_iter=2), two)
    if (one.status != 0).any() or (two.status != 0).any():
        raise AssertionError('the oracle does not fit the unedited cluster: %s %s' % (one.status, two.status))
    return shift_of(one.params_out, one.params, cols).max(), shift_of(two.params_out, one.params_out, cols).max()


def build_calls(oracle, cell, case):
    """The calls of one case of a cell, every oracle result in them (the batches ARE the oracle's
    outputs; clone() one for the engine).  Raises where an expectation is not stable."""
    prep = case.prepare(compute_error=True)
    problem, cols = prep.problem, Columns(prep.problem)
    c, pad = case_cluster(cell), case_pad(cell)
    what = D.cell_id(cell)
    tried = []
    for nudged in NUDGES + ('settled',):
        base = clone(prep.batch)
        r = rows_of(base, c)
        if nudged == 'settled':
            # (a lowpass moves every feature of a large cluster a little in the second round, however
            # the starts are shifted as a whole: every start on the fit of the drawn starts, and the
            # last feature SETTLED_OFF beside it -- one feature moves in round one, none in round two)
            fit = copies(base, c, 1)
            oracle.run_batch(problem, fit)
            delta = fit.params_out[:, cols.pos[0]:cols.pos[-1] + 1] - fit.params[:, cols.pos[0]:cols.pos[-1] + 1]
            delta[-1, -1] += SETTLED_OFF
        else:
            delta = np.zeros((r.stop - r.start, cols.nd))
            delta[:, -1] = nudged
        for name in ('params', 'low', 'high'):
            getattr(base, name)[r, cols.pos[0]:cols.pos[-1] + 1] += delta
        first, second = round_shifts(oracle, problem, base, c, cols)
        tried.append((nudged, first, second))
        if first > 2 * SMALL_SHIFT and second < SMALL_SHIFT / 2:
            break
    else:
        raise AssertionError('%s: no start with round shifts clear of max_shift %.3g: %s' % (what, SMALL_SHIFT, tried))
    pc, names = per_cluster_call(base, c, cols, pad)
    oracle.run_batch(problem, pc)
    alone = copies(base, c, 2 + pad)
    oracle.run_batch(problem, alone)
    if alone.status[0] != 0:
        raise AssertionError('%s: the oracle does not fit the unedited cluster' % what)
    k = names.index('bound_active')
    if pc.status[k] != 0:
        raise AssertionError('%s: bound_active ends with status %d in the oracle' % (what, pc.status[k]))
    # whether bound_active and start_clipped take a second round is decided by a first-round shift
    # against max_shift: it must be clear of it
    probe = copies(pc, k, 1), copies(pc, names.index('start_clipped'), 1)
    for hb in probe:
        oracle.run_batch(with_settings(problem, max_iter=1), hb)
        s = shift_of(hb.params_out, hb.params, cols) / problem.max_shift
        if hb.status[0] != 0 or (np.abs(s - 1.) < SHIFT_CLEAR).any():
            raise AssertionError('%s: first-round shifts %s x max_shift (status %d)' % (what, s, hb.status[0]))
    per_call = {}
    for name in PER_CALL:
        p = call_problem(problem, name, alone.cost[0])
        hb = copies(base, c, 2 + pad)
        oracle.run_batch(p, hb)
        per_call[name] = (p, hb)
    return Calls(problem, cols, pc, names, alone, 0, per_call, nudged)


_CACHE = {}


def calls_of(oracle, cid):
    """[Calls, ...] of a cell, one per case; computed once per process"""
    if cid not in _CACHE:
        cell = CELLS[cid]
        _CACHE[cid] = [build_calls(oracle, cell, case) for case in D.build_case(cell)]
    return _CACHE[cid]


def prefetch(oracle, cids):
    """calls_of for every cell of cids, the cells on WORKERS threads (the oracle keeps no state
    between calls; each cell's calls are made by one thread, in order)"""
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(WORKERS) as pool:
        return dict(zip(cids, pool.map(lambda cid: calls_of(oracle, cid), cids)))


CELLS = collections.OrderedDict((D.cell_id(c), c) for c in D.launchable_cells())
