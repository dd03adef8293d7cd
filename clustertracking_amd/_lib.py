"""ctypes binding of ``libctrefine.so`` (the HIP engine, C-ABI ``include/ctrefine.h``).

There is no CPU fallback: if the library is missing, or no MI355X is visible,
the calls raise.
"""
import collections
import contextlib
import ctypes as C
import os
import threading

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CTREFINE_LIB') or os.path.join(_HERE, 'csrc', 'libctrefine.so')

_P = C.POINTER
_H = _S = C.c_void_p      # an engine handle; a raw stream handle


def _stage(desc):
    return (C.c_int, [_H, _P(desc), _S])


# every symbol include/ctrefine.h declares: (restype, argtypes)
SIGNATURES = {
    'ctr_abi_version': (C.c_int, []),
    'ctr_create': (C.c_int, [_P(C.c_void_p), C.c_int]),
    'ctr_destroy': (None, [_H]),
    'ctr_last_error': (C.c_char_p, [_H]),
    'ctr_validate_problem': (C.c_int, [_P(_abi.Problem), C.c_char_p, C.c_int]),
    'ctr_cluster_n_vars': (C.c_int, [_P(_abi.Problem), C.c_int]),
    'ctr_cluster_kernel': (C.c_int, [_P(_abi.Problem), C.c_int64, _P(_abi.KernelChoice)]),
    'ctr_refine_batch': (C.c_int, [_H, _P(_abi.Problem), _P(_abi.Batch)]),
    'ctr_plan_create': (C.c_int, [_H, _P(_abi.Problem), C.c_int64, C.c_void_p, _P(C.c_void_p)]),
    'ctr_plan_destroy': (None, [C.c_void_p]),
    'ctr_plan_tail': (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    'ctr_plan_tail_bins': (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32)]),
    'ctr_set_tail_absorb': (C.c_int32, [_H, C.c_int32]),
    'ctr_refine_batch_device': (C.c_int, [_H, C.c_void_p, _P(_abi.Batch), _S]),
    'ctr_frame_max_device': (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, _S]),
    'ctr_synchronize': (C.c_int, [_H, _S]),
    'ctr_last_kernel_ms': (C.c_int, [_H, _P(C.c_double), _P(C.c_double)]),
    'ctr_find_clusters': (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    'ctr_engine_wait_stream': (C.c_int, [_H, _S]),
    'ctr_stream_wait_engine': (C.c_int, [_H, _S]),
    'ctr_draw_frames_device': (C.c_int, [_H, _P(_abi.Synth), C.c_void_p, _S]),
    'ctr_locate_maxima_device': _stage(_abi.Locate),
    'ctr_characterize_device': _stage(_abi.Characterize),
    'ctr_link_device': _stage(_abi.Link),
    'ctr_link_adaptive_device': _stage(_abi.LinkAdaptive),
    'ctr_link_predict_device': _stage(_abi.LinkPredict),
    'ctr_preprocess_device': _stage(_abi.Preprocess),
    'ctr_orientation_device': _stage(_abi.Orientation),
    'ctr_diffusion_device': _stage(_abi.Diffusion),
    'ctr_relocate_device': _stage(_abi.Relocate),
    'ctr_relocate_plan': (C.c_int, [_P(_abi.Relocate), _P(C.c_int64), _P(C.c_int64)]),
    'ctr_find_link_device': _stage(_abi.FindLink),
    'ctr_refine_com_device': _stage(_abi.RefineCom),
    'ctr_train_device': _stage(_abi.Train),
    'ctr_refine_global_device': _stage(_abi.RefineGlobal),
    'ctr_refine_global_plan': (C.c_int, [_P(_abi.RefineGlobal), _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), _P(C.c_int64)]),
    'ctr_cluster_tracks_device': _stage(_abi.ClusterTracks),
    'ctr_cluster_tracks_plan': (C.c_int, [_P(_abi.ClusterTracks), _P(C.c_int64), _P(C.c_int32), _P(C.c_int32)]),
    'ctr_track_positions_device': _stage(_abi.TrackPositions),
    'ctr_drift_device': _stage(_abi.Drift),
    'ctr_drift_subtract_device': _stage(_abi.DriftSubtract),
    'ctr_filter_stubs_device': _stage(_abi.FilterStubs),
    'ctr_msd_device': _stage(_abi.Msd),
    'ctr_emsd_device': _stage(_abi.Emsd),
    'ctr_vanhove_device': _stage(_abi.Vanhove),
    'ctr_pair_correlation_device': _stage(_abi.PairCorrelation),
    'ctr_neighbors_device': _stage(_abi.Neighbors),
    'ctr_twopoint_device': _stage(_abi.TwoPoint),
    'ctr_shape_device': _stage(_abi.Shape),
    'ctr_shape_dynamics_device': _stage(_abi.ShapeDynamics),
    'ctr_shape_plan': (C.c_int, [_P(_abi.ShapeDynamics), _P(C.c_int32), _P(C.c_int32), _P(C.c_int64), _P(C.c_int64),
                                 _P(C.c_int64)]),
    'ctr_shape_histogram_device': _stage(_abi.ShapeHistogram),
    'ctr_residual_device': _stage(_abi.Residual),
    'ctr_residual_plan': (C.c_int, [_P(_abi.Residual), _P(C.c_int32), _P(C.c_int32), _P(C.c_int64), _P(C.c_int64),
                                    _P(C.c_int64), _P(C.c_int64)]),
    'ctr_fit_error_device': _stage(_abi.FitError),
    'ctr_fit_error_plan': (C.c_int, [_P(_abi.FitError), _P(C.c_int32), _P(C.c_int32), _P(C.c_int64), _P(C.c_int64),
                                     _P(C.c_int64)]),
    'ctr_contacts_device': _stage(_abi.Contacts),
    'ctr_contacts_plan': (C.c_int, [_P(_abi.Contacts), _P(C.c_int64), _P(C.c_int64), _P(C.c_int64)]),
    'ctr_refine_prepare_device': _stage(_abi.RefinePrepare),
    'ctr_refine_prepare_plan': (C.c_int, [_P(_abi.RefinePrepare), _P(C.c_int64)]),
    'ctr_find_link_refine_device': (C.c_int, [_H, _P(_abi.FindLink), _P(_abi.RefineCom), _S]),
    'ctr_diffusion_ci_device': _stage(_abi.DiffusionCI),
    'ctr_diffusion_ci_plan': (C.c_int, [_P(_abi.DiffusionCI), _P(C.c_int32), _P(C.c_int64), _P(C.c_int64),
                                        _P(C.c_int64)]),
    'ctr_set_stage_max_grid': (C.c_int32, [_H, C.c_int32]),
    'ctr_set_lane_limit': (C.c_int32, [C.c_int32, C.c_int32]),
    'ctr_query_done': (C.c_int, [_H]),
    'ctr_ipc_alloc': (C.c_int, [_H, C.c_int64, _P(C.c_void_p), C.c_void_p]),
    'ctr_ipc_open': (C.c_int, [_H, C.c_void_p, _P(C.c_void_p)]),
    'ctr_ipc_probe': (C.c_int, [_H, C.c_void_p, C.c_int64]),
    'ctr_ipc_read': (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64]),
    'ctr_ipc_close': (C.c_int, [_H, C.c_void_p]),
    'ctr_ipc_free': (C.c_int, [_H, C.c_void_p]),
}
EXPORTS = tuple(SIGNATURES)

_lib = None
_lock = threading.Lock()


class EngineError(RuntimeError):
    pass


def _share_hip_runtime_with_torch():
    """One HIP runtime per process: PyTorch-ROCm wheels bundle their own
    libamdhip64.so.7 (+ HSA runtime).  If libctrefine.so pulled in the system
    copy first, a later ``import torch`` would bind to that one and then fail to
    see the GPU.  So when torch is installed, its copy is loaded first and
    libctrefine.so (DT_NEEDED libamdhip64.so.7) binds to it."""
    import importlib.util
    import sys
    if 'torch' in sys.modules:
        return
    try:
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], 'lib', 'libamdhip64.so')
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load the shared library once; raises EngineError when it is absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        _share_hip_runtime_with_torch()
        if not os.path.exists(LIB_PATH):
            raise EngineError(
                "HIP engine not built: %s is missing. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C clustertracking_amd/csrc`. There is no CPU fallback."
                % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        if hasattr(lib, 'ctr_abi_version') and lib.ctr_abi_version() != _abi.ABI_VERSION:
            raise EngineError("libctrefine.so ABI version mismatch")
        missing = [name for name in EXPORTS if not hasattr(lib, name)]
        if missing:
            raise EngineError("%s does not export %s: rebuild it" % (LIB_PATH, ', '.join(missing)))
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
        return lib


def cluster_kernel(problem, n_features):
    """The kernel a cluster of ``n_features`` goes to (``ctr_cluster_kernel``, no device needed):
    an ``_abi.KernelChoice``."""
    out = _abi.KernelChoice()
    rc = load().ctr_cluster_kernel(C.byref(problem), int(n_features), C.byref(out))
    if rc != _abi.OK:
        raise ValueError("ctr_cluster_kernel: invalid problem or n_features (%d)" % rc)
    return out


def _plan(symbol, desc, *outs):
    """Calls the plan entry ``symbol`` (no device needed) on ``desc``; returns the values of the
    ctypes out-parameters ``outs``.  ``ValueError`` / ``NotImplementedError`` as the call itself."""
    lib = load()
    rc = getattr(lib, symbol)(C.byref(desc), *[C.byref(o) for o in outs])
    if rc != _abi.OK:
        msg = (lib.ctr_last_error(None) or b'').decode()
        raise (ValueError if rc == _abi.ERR_INVALID else NotImplementedError)(msg)
    return tuple(o.value for o in outs)


def relocate_plan(desc):
    """(pixels of the LDS tile, dynamic LDS bytes) of a ``ctr_relocate_device`` launch
    (``ctr_relocate_plan``, no device needed); ``ValueError`` / ``NotImplementedError`` as the call itself."""
    return _plan('ctr_relocate_plan', desc, C.c_int64(), C.c_int64())


def diffusion_ci_plan(desc):
    """The launch decision of ``ctr_diffusion_ci_device`` (``ctr_diffusion_ci_plan``, no device needed):
    ``(rows_in_lds, lds_bytes, scratch_bytes, pairs_per_chunk)``; ``ValueError`` /
    ``NotImplementedError`` as the call itself."""
    in_lds, lds, scratch, chunk = _plan('ctr_diffusion_ci_plan', desc, C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64())
    return bool(in_lds), lds, scratch, chunk


def cluster_tracks_plan(desc):
    """``(scratch_bytes, max_rounds, jumps_per_round)`` of a ``ctr_cluster_tracks_device`` call
    (``ctr_cluster_tracks_plan``, no device needed); ``ValueError`` / ``NotImplementedError`` as the call itself."""
    return _plan('ctr_cluster_tracks_plan', desc, C.c_int64(), C.c_int32(), C.c_int32())


def shape_plan(desc):
    """The launch decision of ``ctr_shape_dynamics_device`` (``ctr_shape_plan``, no device needed):
    ``(tile, halo, lds_bytes, n_tiles, scratch_bytes)``; ``ValueError`` as the call itself."""
    return _plan('ctr_shape_plan', desc, C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64())


ResidualPlan = collections.namedtuple('ResidualPlan', 'tile chunk n_tiles grids lds_bytes scratch_bytes')


def residual_plan(desc):
    """The launch decision of ``ctr_residual_device`` (``ctr_residual_plan``, no device needed):
    ``ResidualPlan(tile (3 ints), chunk, n_tiles, grids (check, frame, feature, cluster), lds_bytes,
    scratch_bytes)``; ``ValueError`` / ``NotImplementedError`` as the call itself."""
    lib = load()
    tile, grids = (C.c_int32 * 3)(), (C.c_int64 * 4)()
    chunk, n_tiles, lds, scratch = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib.ctr_residual_plan(C.byref(desc), tile, C.byref(chunk), C.byref(n_tiles), grids, C.byref(lds), C.byref(scratch))
    if rc != _abi.OK:
        msg = (lib.ctr_last_error(None) or b'').decode()
        raise (ValueError if rc == _abi.ERR_INVALID else NotImplementedError)(msg)
    return ResidualPlan(tuple(tile), chunk.value, n_tiles.value, tuple(grids), lds.value, scratch.value)


FitErrorPlan = collections.namedtuple('FitErrorPlan', 'max_vars chunk lds_bytes grid scratch_bytes')


def fit_error_plan(desc):
    """The launch decision of ``ctr_fit_error_device`` (``ctr_fit_error_plan``, no device needed):
    ``FitErrorPlan(max_vars, chunk, lds_bytes (one entry per size class), grid, scratch_bytes)``;
    ``ValueError`` / ``NotImplementedError`` as the call itself."""
    lib = load()
    k = _abi.FITERR_CLASSES
    max_vars, chunk, lds = (C.c_int32 * k)(), (C.c_int32 * k)(), (C.c_int64 * k)()
    grid, scratch = C.c_int64(), C.c_int64()
    rc = lib.ctr_fit_error_plan(C.byref(desc), max_vars, chunk, lds, C.byref(grid), C.byref(scratch))
    if rc != _abi.OK:
        msg = (lib.ctr_last_error(None) or b'').decode()
        raise (ValueError if rc == _abi.ERR_INVALID else NotImplementedError)(msg)
    return FitErrorPlan(tuple(max_vars), tuple(chunk), tuple(lds), grid.value, scratch.value)


ContactsPlan = collections.namedtuple('ContactsPlan', 'scratch_bytes scan_tiles grids')


def contacts_plan(desc):
    """The launch decision of ``ctr_contacts_device`` (``ctr_contacts_plan``, no device needed):
    ``ContactsPlan(scratch_bytes, scan_tiles (rows, entries), grids (check, walk, entries, chains))``;
    ``ValueError`` as the call itself."""
    lib = load()
    scratch, tiles, grids = C.c_int64(), (C.c_int64 * 2)(), (C.c_int64 * 4)()
    rc = lib.ctr_contacts_plan(C.byref(desc), C.byref(scratch), tiles, grids)
    if rc != _abi.OK:
        msg = (lib.ctr_last_error(None) or b'').decode()
        raise (ValueError if rc == _abi.ERR_INVALID else NotImplementedError)(msg)
    return ContactsPlan(scratch.value, tuple(tiles), tuple(grids))


RefineGlobalPlan = collections.namedtuple('RefineGlobalPlan', 'scratch_bytes launches_per_iteration tiles row_doubles')


def refine_global_plan(desc):
    """The launch decision of ``ctr_refine_global_device`` (``ctr_refine_global_plan``, no device
    needed): ``RefineGlobalPlan(scratch_bytes, launches_per_iteration, tiles, row_doubles)``;
    ``ValueError`` / ``NotImplementedError`` as the call itself."""
    return RefineGlobalPlan(*_plan('ctr_refine_global_plan', desc, C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()))


def refine_prepare_plan(desc):
    """Scratch bytes of a ``ctr_refine_prepare_device`` call (``ctr_refine_prepare_plan``, no device
    needed); ``ValueError`` / ``NotImplementedError`` as the call itself."""
    return _plan('ctr_refine_prepare_plan', desc, C.c_int64())[0]


class Engine(object):
    """One engine handle bound to one GPU (``ctr_create`` / ``ctr_destroy``)."""

    def __init__(self, device=0):
        self._lib = load()
        self._h = C.c_void_p()
        rc = self._lib.ctr_create(C.byref(self._h), int(device))
        if rc != _abi.OK:
            msg = self._lib.ctr_last_error(None)
            self._h = None
            raise EngineError("ctr_create(device=%d) failed (%d): %s" % (
                device, rc, (msg or b'').decode()))
        self.device = int(device)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.ctr_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc, what, too_large=False):
        """``too_large``: CTR_ERR_UNSUPPORTED of this entry point means a size beyond the device
        path (an LDS tile over 64 KiB), not a missing feature: ``EngineError``."""
        if rc != _abi.OK:
            msg = (self._lib.ctr_last_error(self._h) or b'').decode()
            if rc == _abi.ERR_INVALID:
                raise ValueError("%s: %s" % (what, msg))
            if rc == _abi.ERR_UNSUPPORTED and too_large:
                raise EngineError("%s: %s" % (what, msg))
            if rc == _abi.ERR_UNSUPPORTED:
                raise NotImplementedError("%s: %s" % (what, msg))
            raise EngineError("%s failed (%d): %s" % (what, rc, msg))

    def refine_batch(self, problem, batch):
        """Host-buffer call: ``batch`` is an ``_abi.HostBatch``; outputs are
        written into its arrays."""
        b = batch.as_struct()
        self._check(self._lib.ctr_refine_batch(self._h, C.byref(problem), C.byref(b)),
                    'ctr_refine_batch')
        return batch

    # ---- device-resident path (bench, multi-GPU driver) ---------------------
    def plan(self, problem, feat_offset_host):
        import numpy as np
        off = np.ascontiguousarray(feat_offset_host, dtype=np.int32)
        plan = C.c_void_p()
        self._check(self._lib.ctr_plan_create(self._h, C.byref(problem), len(off) - 1,
                                              off.ctypes.data, C.byref(plan)),
                    'ctr_plan_create')
        return Plan(self._lib, plan)

    def set_tail_absorb(self, max_count):
        """``ctr_set_tail_absorb``: the most clusters of a 3-4- or 5-10-feature bin that the tail
        launch of a plan made from now on fits whole (0: never); returns the previous value.  A
        negative ``max_count`` only asks."""
        return int(self._lib.ctr_set_tail_absorb(self._h, int(max_count)))

    def refine_batch_device(self, plan, batch_struct, stream=None):
        self._check(self._lib.ctr_refine_batch_device(
            self._h, plan._p, C.byref(batch_struct), C.c_void_p(stream or 0)),
            'ctr_refine_batch_device')

    def frame_max_device(self, frames_ptr, dtype_code, n_frames, frame_elems, out_ptr,
                         stream=None):
        self._check(self._lib.ctr_frame_max_device(
            self._h, C.c_void_p(frames_ptr), dtype_code, n_frames, frame_elems,
            C.c_void_p(out_ptr), C.c_void_p(stream or 0)), 'ctr_frame_max_device')

    def find_clusters(self, pos, frame_offset, separation):
        """Labels (smallest row index of the cluster) and sizes for a frame-sorted
        position table; ``ctr_find_clusters``."""
        import numpy as np
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        off = np.ascontiguousarray(frame_offset, dtype=np.int32)
        sep = np.ascontiguousarray(separation, dtype=np.float64)
        n, nd = pos.shape
        labels = np.empty(n, dtype=np.int32)
        sizes = np.empty(n, dtype=np.int32)
        self._check(self._lib.ctr_find_clusters(self._h, nd, pos.ctypes.data, off.ctypes.data,
                                                len(off) - 1, sep.ctypes.data,
                                                labels.ctypes.data, sizes.ctypes.data),
                    'ctr_find_clusters')
        return labels, sizes

    def draw_frames_device(self, synth, frames_ptr, stream=None):
        """``ctr_draw_frames_device``: ``synth`` is an ``_abi.Synth`` with device pointers."""
        self._check(self._lib.ctr_draw_frames_device(self._h, C.byref(synth), C.c_void_p(frames_ptr),
                                                     C.c_void_p(stream or 0)), 'ctr_draw_frames_device')

    def query_done(self):
        """True when the last ``refine_batch_device`` call of this engine has finished on the
        device (``ctr_query_done``; never blocks)."""
        rc = self._lib.ctr_query_done(self._h)
        if rc < 0:
            raise EngineError("ctr_query_done failed: %s" % (self._lib.ctr_last_error(self._h) or b'').decode())
        return rc == 1

    def set_stage_max_grid(self, max_grid):
        """``ctr_set_stage_max_grid``: the cap on the grids of the table stages' grid-stride kernels
        for every later stage call of this engine (1 .. 65536; 0: the default, 65536).  Returns the
        cap before, -1 for a value outside the range (nothing changes)."""
        return int(self._lib.ctr_set_stage_max_grid(self._h, C.c_int32(int(max_grid))))

    @contextlib.contextmanager
    def stage_max_grid(self, max_grid):
        """A test switch: inside the ``with`` block the table stages launch their grid-stride
        kernels with at most ``max_grid`` workgroups, so that small tables take the trips past the
        grid; results never depend on it.  The cap before is restored on the way out, also after
        an exception: the default engine is shared by every call of the process."""
        before = self.set_stage_max_grid(max_grid)
        if before < 0:
            raise ValueError("stage_max_grid: %r is outside [0, 65536]" % (max_grid,))
        try:
            yield self
        finally:
            self.set_stage_max_grid(before)

    def set_lane_limit(self, n):
        """``ctr_set_lane_limit`` on this engine's device: later ``refine_batch_device`` calls use
        only the first ``n`` lanes (0: all).  Returns the number in use before, -1 for a value
        outside the range (nothing changes).  Results never depend on it."""
        return int(self._lib.ctr_set_lane_limit(C.c_int32(self.device), C.c_int32(int(n))))

    def synchronize(self, stream=None):
        self._check(self._lib.ctr_synchronize(self._h, C.c_void_p(stream or 0)),
                    'ctr_synchronize')

    # ---- the inbox of a multi-GPU pipeline (include/ctrefine.h: ctr_ipc_*) ---------------------
    def ipc_alloc(self, n_bytes):
        """(device pointer, handle blob) of a zeroed block on this engine's device that other
        processes can map (the blob names the owning device, include/ctrefine.h)."""
        ptr = C.c_void_p()
        handle = (C.c_ubyte * _abi.IPC_HANDLE_BYTES)()
        self._check(self._lib.ctr_ipc_alloc(self._h, C.c_int64(int(n_bytes)), C.byref(ptr), handle), 'ctr_ipc_alloc')
        return int(ptr.value), bytes(handle)

    def ipc_open(self, handle):
        ptr = C.c_void_p()
        if len(handle) != _abi.IPC_HANDLE_BYTES:
            raise ValueError("an inbox handle has %d bytes" % _abi.IPC_HANDLE_BYTES)
        buf = (C.c_ubyte * _abi.IPC_HANDLE_BYTES).from_buffer_copy(handle)
        self._check(self._lib.ctr_ipc_open(self._h, buf, C.byref(ptr)), 'ctr_ipc_open')
        return int(ptr.value)

    def ipc_probe(self, ptr, value):
        self._check(self._lib.ctr_ipc_probe(self._h, C.c_void_p(int(ptr)), C.c_int64(int(value))), 'ctr_ipc_probe')

    def ipc_read(self, ptr, shape, dtype):
        import numpy as np
        out = np.empty(shape, dtype=dtype)
        self._check(self._lib.ctr_ipc_read(self._h, C.c_void_p(out.ctypes.data), C.c_void_p(int(ptr)),
                                           C.c_int64(out.nbytes)), 'ctr_ipc_read')
        return out

    def ipc_close(self, ptr):
        self._check(self._lib.ctr_ipc_close(self._h, C.c_void_p(int(ptr))), 'ctr_ipc_close')

    def ipc_free(self, ptr):
        self._check(self._lib.ctr_ipc_free(self._h, C.c_void_p(int(ptr))), 'ctr_ipc_free')

    def engine_wait_stream(self, stream=0):
        """The engine's own stream waits (on the device) for what is queued on ``stream``
        (raw handle; 0 = the legacy default stream)."""
        self._check(self._lib.ctr_engine_wait_stream(self._h, C.c_void_p(stream or 0)),
                    'ctr_engine_wait_stream')

    def stream_wait_engine(self, stream=0):
        """``stream`` waits (on the device) for what is queued on the engine's own stream."""
        self._check(self._lib.ctr_stream_wait_engine(self._h, C.c_void_p(stream or 0)),
                    'ctr_stream_wait_engine')

    def on_current_stream(self, call, *args, dev):
        """``call(*args, stream)`` in order with torch's current stream on ``dev``: on that stream,
        or, where that is the legacy default stream (handle 0, which to the engine means its own
        stream), on the engine's stream, ordered with the default stream by events on the device."""
        import torch
        stream = torch.cuda.current_stream(dev).cuda_stream
        if stream:
            call(*args, stream)
        else:
            self.engine_wait_stream(0)
            call(*args, 0)
            self.stream_wait_engine(0)

    def find_link_refine_device(self, desc, com, stream=None):
        """``ctr_find_link_refine_device``: ``desc`` an ``_abi.FindLink``, ``com`` an ``_abi.RefineCom``
        (raw frames, ``max_iterations``, ``shift_thresh``), device pointers."""
        self._check(self._lib.ctr_find_link_refine_device(self._h, C.byref(desc), C.byref(com),
                                                          C.c_void_p(stream or 0)), 'ctr_find_link_refine_device')

    def last_kernel_ms(self):
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.ctr_last_kernel_ms(self._h, C.byref(a), C.byref(b)),
                    'ctr_last_kernel_ms')
        return a.value, b.value


def _stage_method(symbol, too_large):
    def method(self, desc, stream=None):
        self._check(getattr(self._lib, symbol)(self._h, C.byref(desc), C.c_void_p(stream or 0)),
                    symbol, too_large=too_large)
    method.__doc__ = "``%s``: ``desc`` is its ``_abi`` descriptor with device pointers." % symbol
    return method


# the stage calls ``Engine.<name>(desc, stream=None)``: (name, symbol, too_large of Engine._check)
for _name, _symbol, _too_large in (
        ('locate_maxima_device', 'ctr_locate_maxima_device', True),
        ('characterize_device', 'ctr_characterize_device', False),
        ('link_device', 'ctr_link_device', False),
        ('link_adaptive_device', 'ctr_link_adaptive_device', False),
        ('link_predict_device', 'ctr_link_predict_device', False),
        ('preprocess_device', 'ctr_preprocess_device', True),
        ('orientation_device', 'ctr_orientation_device', False),
        ('diffusion_device', 'ctr_diffusion_device', False),
        ('diffusion_ci_device', 'ctr_diffusion_ci_device', False),
        ('relocate_device', 'ctr_relocate_device', False),
        ('find_link_device', 'ctr_find_link_device', False),
        ('refine_com_device', 'ctr_refine_com_device', False),
        ('train_device', 'ctr_train_device', False),
        ('refine_global_device', 'ctr_refine_global_device', False),
        ('cluster_tracks_device', 'ctr_cluster_tracks_device', False),
        ('track_positions_device', 'ctr_track_positions_device', False),
        ('drift_device', 'ctr_drift_device', False),
        ('drift_subtract_device', 'ctr_drift_subtract_device', False),
        ('filter_stubs_device', 'ctr_filter_stubs_device', False),
        ('msd_device', 'ctr_msd_device', False),
        ('emsd_device', 'ctr_emsd_device', False),
        ('vanhove_device', 'ctr_vanhove_device', False),
        ('pair_correlation_device', 'ctr_pair_correlation_device', False),
        ('neighbors_device', 'ctr_neighbors_device', False),
        ('twopoint_device', 'ctr_twopoint_device', False),
        ('shape_device', 'ctr_shape_device', False),
        ('shape_dynamics_device', 'ctr_shape_dynamics_device', False),
        ('shape_histogram_device', 'ctr_shape_histogram_device', False),
        ('residual_device', 'ctr_residual_device', False),
        ('contacts_device', 'ctr_contacts_device', False),
        ('fit_error_device', 'ctr_fit_error_device', False),
        ('refine_prepare_device', 'ctr_refine_prepare_device', False)):
    setattr(Engine, _name, _stage_method(_symbol, _too_large))


class Plan(object):
    def __init__(self, lib, p):
        self._lib, self._p = lib, p

    def close(self):
        if self._p:
            self._lib.ctr_plan_destroy(self._p)
            self._p = None

    def tail(self):
        """``ctr_plan_tail``: ``(fused, cap, tail_grid)`` -- whether the plan fits the likely slow
        clusters of its pairs, 3-4-feature and 5-10-feature bins in one tail launch, the most
        entries of a bin that launch takes, and its workgroups (0 if not fused)."""
        fused, cap, grid = C.c_int32(), C.c_int32(), C.c_int32()
        rc = self._lib.ctr_plan_tail(self._p, C.byref(fused), C.byref(cap), C.byref(grid))
        if rc != _abi.OK:
            raise ValueError("ctr_plan_tail: no plan (%d)" % rc)
        return bool(fused.value), int(cap.value), int(grid.value)

    def tail_bins(self):
        """``ctr_plan_tail_bins``: ``(absorbed, own_launch)``, each three booleans -- pairs,
        3-4-feature, 5-10-feature bin: whether the tail launch fits the whole bin, and whether
        the bin's own launch (pairs: the 64-lane one) is queued."""
        absorbed, own = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        rc = self._lib.ctr_plan_tail_bins(self._p, absorbed, own)
        if rc != _abi.OK:
            raise ValueError("ctr_plan_tail_bins: no plan (%d)" % rc)
        return tuple(bool(v) for v in absorbed), tuple(bool(v) for v in own)

    __del__ = close


_default_engines = {}


def default_engine(device=0):
    eng = _default_engines.get(device)
    if eng is None:
        eng = _default_engines[device] = Engine(device)
    return eng
