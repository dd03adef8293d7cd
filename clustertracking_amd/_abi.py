"""ctypes mirror of ``include/ctrefine.h`` and the host-side batch container.

Pure description of the C-ABI (structs, enums) plus a NumPy container for one
batch of clusters.  No arithmetic.
"""
import ctypes as C

import numpy as np

ABI_VERSION = 8
IPC_HANDLE_BYTES = 128
MAX_NDIM = 3
MAX_NOISE_SIZE = 4.0
MAX_PARAMS = 12
MAX_VARS = 127

OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_DEVICE, ERR_NOMEM = range(5)

DTYPE_CODES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int16): 2,
               np.dtype(np.int32): 3, np.dtype(np.float32): 4, np.dtype(np.float64): 5}

FIT_GAUSS, FIT_RING, FIT_DISC, FIT_INV_SERIES = 0, 1, 2, 3
FIT_CODES = {'gauss': FIT_GAUSS, 'ring': FIT_RING, 'disc': FIT_DISC}
FIT_EXTRAS = {FIT_GAUSS: 0, FIT_RING: 1, FIT_DISC: 1}   # profile parameters after the sizes


def fit_code(fit_function):
    """(CTR_FIT_* code, number of profile parameters) of a fit function name; ``'inv_series_<N>'``
    has N + 1 of them (fitfunc.py:334-343)."""
    if fit_function in FIT_CODES:
        code = FIT_CODES[fit_function]
        return code, FIT_EXTRAS[code]
    head, _, order = str(fit_function).rpartition('_')
    if head == 'inv_series' and order.isdigit():
        return FIT_INV_SERIES, int(order) + 1
    raise ValueError("fit_function must be one of %s or 'inv_series_<N>'" % sorted(FIT_CODES))
MODE_CONST, MODE_VAR, MODE_GLOBAL, MODE_CLUSTER = 0, 1, 2, 3
CONS_NONE, CONS_DIMER, CONS_TRIMER, CONS_TETRAMER = 0, 1, 2, 3
CONS_CODES = {None: 0, 'dimer': 1, 'trimer': 2, 'tetramer': 3}

STATUS_OK = 0
STATUS_OUT_OF_BOUNDS = 1
STATUS_NONFINITE = 2
STATUS_NO_CONVERGENCE = 3
STATUS_RMS_DEV = 4
STATUS_TOO_LARGE = 5
STATUS_TEXT = {
    0: 'ok',
    1: 'coordinates are out of image bounds',
    2: 'non-finite initial parameters',
    3: 'solver did not converge',
    4: 'rms deviation of the fit is more than max_rms_dev',
    5: 'cluster is beyond the engine (a feature with more than 48 overlapping neighbours)',
}


# ctr_cluster_kernel (include/ctrefine.h): the kernel a cluster goes to
KBIN_SMALL1, KBIN_SMALL2, KBIN_BLOCK, KBIN_CONS, KBIN_LARGE, KBIN_TOO_LARGE = 1, 2, 3, 4, 5, 6
KFAM_NONE, KFAM_SMALL, KFAM_GAUSS, KFAM_GAUSS_TP, KFAM_LOWPASS, KFAM_RING, KFAM_DISC, \
    KFAM_INV_SERIES, KFAM_LARGE, KFAM_LARGE_LOWPASS = range(10)


FLAG_THROUGHPUT = 1   # ctr_problem.flags (include/ctrefine.h): scheduling hint, results unchanged
FLAG_ISOLATE_TAIL = 2  # accepted, without effect: the lanes place a long kernel by its measured duration
FLAG_WINDOW_FILTER = 4  # noise_size was given: the window is thresholded even with every sigma 0


class Problem(C.Structure):
    _fields_ = [
        ('ndim', C.c_int32), ('isotropic', C.c_int32), ('fit_function', C.c_int32),
        ('n_params', C.c_int32), ('modes', C.c_int32 * MAX_PARAMS),
        ('radius', C.c_int32 * MAX_NDIM), ('constraint_kind', C.c_int32),
        ('max_iter', C.c_int32), ('solver_maxiter', C.c_int32), ('flags', C.c_int32),
        ('constraint_dist', C.c_double * MAX_NDIM), ('max_shift', C.c_double),
        ('max_rms_dev', C.c_double), ('residual_factor', C.c_double),
        ('xtol', C.c_double), ('ftol', C.c_double), ('threshold', C.c_double),
        ('noise_size', C.c_double * MAX_NDIM),
    ]


class Batch(C.Structure):
    _fields_ = [
        ('frames', C.c_void_p), ('frame_dtype', C.c_int32), ('reserved0', C.c_int32),
        ('n_frames', C.c_int64), ('shape', C.c_int64 * MAX_NDIM),
        ('n_clusters', C.c_int64), ('n_features', C.c_int64),
        ('frame_index', C.c_void_p), ('feat_offset', C.c_void_p),
        ('params', C.c_void_p), ('low', C.c_void_p), ('high', C.c_void_p),
        ('params_out', C.c_void_p), ('cost', C.c_void_p), ('status', C.c_void_p),
        ('n_rounds', C.c_void_p), ('n_iter', C.c_void_p), ('params_std', C.c_void_p),
        ('result_rows', C.c_void_p), ('done_flag', C.c_void_p), ('done_value', C.c_int64),
    ]


class KernelChoice(C.Structure):
    """``ctr_kernel_choice`` (include/ctrefine.h)."""
    _fields_ = [('bin', C.c_int32), ('family', C.c_int32), ('nt', C.c_int32),
                ('lanes', C.c_int32), ('n_vars', C.c_int32), ('reserved0', C.c_int32)]


class Synth(C.Structure):
    """``ctr_synth`` (include/ctrefine.h): synthetic frames on the device."""
    _fields_ = [
        ('ndim', C.c_int32), ('frame_dtype', C.c_int32), ('n_frames', C.c_int64),
        ('shape', C.c_int64 * MAX_NDIM), ('n_features', C.c_int64),
        ('frame_of', C.c_void_p), ('pos', C.c_void_p), ('size', C.c_void_p),
        ('max_value', C.c_void_p), ('noise', C.c_double), ('seed', C.c_uint64),
    ]


class Locate(C.Structure):
    """``ctr_locate`` (include/ctrefine.h): feature location on the device."""
    _fields_ = [
        ('ndim', C.c_int32), ('frame_dtype', C.c_int32), ('n_frames', C.c_int64),
        ('shape', C.c_int64 * MAX_NDIM), ('separation', C.c_double * MAX_NDIM),
        ('percentile', C.c_double), ('margin', C.c_int64 * MAX_NDIM),
        ('precise', C.c_int32), ('reserved0', C.c_int32), ('capacity', C.c_int64),
        ('frames', C.c_void_p), ('frame_offset', C.c_void_p), ('pos_out', C.c_void_p),
        ('total', C.c_void_p), ('threshold', C.c_void_p),
    ]


class Characterize(C.Structure):
    """``ctr_characterize`` (include/ctrefine.h): mass, signal and size of located features."""
    _fields_ = [
        ('ndim', C.c_int32), ('frame_dtype', C.c_int32), ('n_frames', C.c_int64),
        ('shape', C.c_int64 * MAX_NDIM), ('radius', C.c_int64 * MAX_NDIM),
        ('isotropic', C.c_int32), ('reserved0', C.c_int32), ('scale_factor', C.c_double),
        ('frames', C.c_void_p), ('n_features', C.c_int64), ('frame_offset', C.c_void_p),
        ('pos', C.c_void_p), ('pos_i32', C.c_void_p),
        ('mass', C.c_void_p), ('signal', C.c_void_p), ('size', C.c_void_p),
    ]


PRE_LOWPASS, PRE_BANDPASS, PRE_PREPROCESS, PRE_SCALE = 0, 1, 2, 3   # ctr_preprocess.mode
PRE_AUTO, PRE_BAND_PLANE, PRE_TWICE = 0, 1, 2                        # ctr_preprocess.strategy


class Preprocess(C.Structure):
    """``ctr_preprocess`` (include/ctrefine.h): bandpass, lowpass and rescaling of whole frames."""
    _fields_ = [
        ('ndim', C.c_int32), ('frame_dtype', C.c_int32), ('n_frames', C.c_int64),
        ('shape', C.c_int64 * MAX_NDIM), ('mode', C.c_int32), ('strategy', C.c_int32),
        ('n_taps', C.c_int32 * MAX_NDIM), ('box', C.c_int32 * MAX_NDIM),
        ('taps', C.c_void_p * MAX_NDIM), ('threshold', C.c_double),
        ('frames', C.c_void_p), ('out', C.c_void_p), ('scale_factor', C.c_void_p),
    ]


LINK_OK, LINK_OVERSIZE, LINK_CAPACITY = 0, 1, 2   # ctr_link.status[0]
LINK_MAX_SOURCES, LINK_MAX_DESTINATIONS = 30, 64


class Link(C.Structure):
    """``ctr_link`` (include/ctrefine.h): frame-to-frame linking on the device."""
    _fields_ = [
        ('ndim', C.c_int32), ('memory', C.c_int32), ('n_levels', C.c_int64),
        ('n_features', C.c_int64), ('search_range', C.c_double * MAX_NDIM),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('particle', C.c_void_p),
        ('n_tracks', C.c_void_p), ('status', C.c_void_p),
    ]


LINK_MAX_ROUNDS = 64


class LinkAdaptive(C.Structure):
    """``ctr_link_adaptive`` (include/ctrefine.h): linking with an adaptive search range."""
    _fields_ = Link._fields_ + [
        ('stop_rel', C.c_double), ('step', C.c_double), ('max_rounds', C.c_int32),
        ('adaptive_round', C.c_void_p),
    ]


LINK_PREDICT_VELOCITY, LINK_PREDICT_DRIFT = 1, 2   # ctr_link_predict.predictor


class LinkPredict(C.Structure):
    """``ctr_link_predict`` (include/ctrefine.h): linking with a velocity or drift prediction;
    ``max_rounds == 0``: no adaptive search range."""
    _fields_ = LinkAdaptive._fields_ + [
        ('predictor', C.c_int32), ('initial_velocity', C.c_double * MAX_NDIM), ('velocity', C.c_void_p),
    ]


RELOCATE_OK, RELOCATE_CAPACITY, RELOCATE_BAD_FRAME = 0, 1, 2  # ctr_relocate.status[q]
RELOCATE_MAX_MAXIMA, RELOCATE_MAX_BACKGROUND, RELOCATE_TILE_BYTES = 256, 512, 32768


class Relocate(C.Structure):
    """``ctr_relocate`` (include/ctrefine.h): relocation candidates of lost features on the device."""
    _fields_ = [
        ('ndim', C.c_int32), ('frame_dtype', C.c_int32), ('n_frames', C.c_int64),
        ('shape', C.c_int64 * MAX_NDIM), ('radius', C.c_int64 * MAX_NDIM),
        ('separation', C.c_double * MAX_NDIM), ('search_range', C.c_double * MAX_NDIM),
        ('isotropic', C.c_int32), ('max_candidates', C.c_int32),
        ('minmass', C.c_double), ('scale_factor', C.c_double),
        ('frames', C.c_void_p), ('threshold', C.c_void_p),
        ('n_known', C.c_int64), ('known_pos', C.c_void_p), ('known_offset', C.c_void_p),
        ('n_queries', C.c_int64), ('query_frame', C.c_void_p), ('source_offset', C.c_void_p),
        ('source_pos', C.c_void_p),
        ('n_found', C.c_void_p), ('cand_pos', C.c_void_p), ('mass', C.c_void_p),
        ('signal', C.c_void_p), ('size', C.c_void_p), ('status', C.c_void_p),
    ]


FIND_LINK_OK, FIND_LINK_OVERSIZE, FIND_LINK_CAPACITY = 0, 1, 2   # ctr_find_link.status[0]
FIND_LINK_RELOCATE, FIND_LINK_QUERIES, FIND_LINK_ROWS = 3, 4, 5


class FindLink(C.Structure):
    """``ctr_find_link`` (include/ctrefine.h): find and link with relocation on the device."""
    _fields_ = [
        ('ndim', C.c_int32), ('frame_dtype', C.c_int32), ('n_frames', C.c_int64),
        ('shape', C.c_int64 * MAX_NDIM), ('radius', C.c_int64 * MAX_NDIM),
        ('separation', C.c_double * MAX_NDIM), ('search_range', C.c_double * MAX_NDIM),
        ('isotropic', C.c_int32), ('memory', C.c_int32),
        ('max_queries', C.c_int32), ('max_relocated', C.c_int32),
        ('minmass', C.c_double), ('scale_factor', C.c_double),
        ('frames', C.c_void_p), ('threshold', C.c_void_p),
        ('n_located', C.c_int64), ('pos', C.c_void_p), ('frame_offset', C.c_void_p),
        ('mass', C.c_void_p), ('signal', C.c_void_p), ('size', C.c_void_p),
        ('capacity', C.c_int64), ('pos_out', C.c_void_p), ('frame_offset_out', C.c_void_p),
        ('particle', C.c_void_p), ('mass_out', C.c_void_p), ('signal_out', C.c_void_p),
        ('size_out', C.c_void_p), ('relocated', C.c_void_p), ('n_tracks', C.c_void_p),
        ('coupled', C.c_void_p), ('status', C.c_void_p),
    ]


class RefineCom(C.Structure):
    """``ctr_refine_com`` (include/ctrefine.h): centre-of-mass refinement of features."""
    _fields_ = [
        ('ndim', C.c_int32), ('frame_dtype', C.c_int32), ('n_frames', C.c_int64),
        ('shape', C.c_int64 * MAX_NDIM), ('radius', C.c_int64 * MAX_NDIM),
        ('max_iterations', C.c_int32), ('reserved0', C.c_int32), ('shift_thresh', C.c_double),
        ('frames', C.c_void_p), ('n_features', C.c_int64), ('frame_offset', C.c_void_p),
        ('pos', C.c_void_p), ('pos_out', C.c_void_p), ('mass', C.c_void_p), ('n_iter', C.c_void_p),
    ]


TRAIN_MAX_GLOBALS, TRAIN_MAX_FEATURES = 8, 64


class Train(C.Structure):
    """``ctr_train`` (include/ctrefine.h): training of shared fit parameters on the device."""
    _fields_ = [
        ('ndim', C.c_int32), ('isotropic', C.c_int32), ('fit_function', C.c_int32),
        ('n_params', C.c_int32), ('modes', C.c_int32 * MAX_PARAMS), ('radius', C.c_int32 * MAX_NDIM),
        ('frame_dtype', C.c_int32), ('solver_maxiter', C.c_int32), ('max_features', C.c_int32),
        ('check_every', C.c_int32),
        ('n_frames', C.c_int64), ('shape', C.c_int64 * MAX_NDIM),
        ('n_problems', C.c_int64), ('n_clusters', C.c_int64), ('n_features', C.c_int64),
        ('residual_factor', C.c_double), ('max_rms_dev', C.c_double),
        ('xtol', C.c_double), ('ftol', C.c_double),
        ('frames', C.c_void_p), ('params', C.c_void_p), ('feat_offset', C.c_void_p),
        ('frame_index', C.c_void_p), ('problem_offset', C.c_void_p),
        ('start', C.c_void_p), ('low', C.c_void_p), ('high', C.c_void_p),
        ('globals', C.c_void_p), ('cost', C.c_void_p), ('status', C.c_void_p), ('n_iter', C.c_void_p),
    ]


REFINE_GLOBAL_MAX_GLOBALS, REFINE_GLOBAL_MAX_COLUMNS = 8, 48


class RefineGlobal(C.Structure):
    """``ctr_refine_global`` (include/ctrefine.h): shared and per-feature parameters in one problem."""
    _fields_ = [
        ('ndim', C.c_int32), ('isotropic', C.c_int32), ('fit_function', C.c_int32),
        ('n_params', C.c_int32), ('modes', C.c_int32 * MAX_PARAMS), ('radius', C.c_int32 * MAX_NDIM),
        ('frame_dtype', C.c_int32), ('solver_maxiter', C.c_int32), ('max_iter', C.c_int32),
        ('max_features', C.c_int32), ('max_locals', C.c_int32), ('check_every', C.c_int32),
        ('reserved0', C.c_int32),
        ('n_frames', C.c_int64), ('shape', C.c_int64 * MAX_NDIM),
        ('n_problems', C.c_int64), ('n_clusters', C.c_int64), ('n_features', C.c_int64),
        ('residual_factor', C.c_double), ('max_rms_dev', C.c_double), ('max_shift', C.c_double),
        ('xtol', C.c_double), ('ftol', C.c_double),
        ('frames', C.c_void_p), ('params', C.c_void_p), ('feat_offset', C.c_void_p),
        ('frame_index', C.c_void_p), ('problem_offset', C.c_void_p),
        ('start', C.c_void_p), ('low', C.c_void_p), ('high', C.c_void_p),
        ('local_start', C.c_void_p), ('local_low', C.c_void_p), ('local_high', C.c_void_p),
        ('params_out', C.c_void_p), ('globals', C.c_void_p), ('cost', C.c_void_p), ('status', C.c_void_p),
        ('n_rounds', C.c_void_p), ('n_iter', C.c_void_p),
    ]


TRACKS_PAIRS, TRACKS_COMPONENTS = 0, 1                        # ctr_cluster_tracks.phase
TRACKS_OK, TRACKS_BAD_TABLE, TRACKS_ROUNDS = 0, 1, 2           # status[0] of both calls
TRACKS_NO_KEY = 0x7fffffffffffffff


class ClusterTracks(C.Structure):
    """``ctr_cluster_tracks`` (include/ctrefine.h): which particles form one cluster over time."""
    _fields_ = [
        ('phase', C.c_int32), ('cluster_size', C.c_int32), ('check_every', C.c_int32), ('reserved0', C.c_int32),
        ('min_frames', C.c_int64), ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_particles', C.c_int64),
        ('frame_offset', C.c_void_p), ('particle', C.c_void_p), ('cluster', C.c_void_p), ('keys', C.c_void_p),
        ('track_of_particle', C.c_void_p), ('n_tracks', C.c_void_p), ('n_members', C.c_void_p),
        ('status', C.c_void_p), ('n_rounds', C.c_void_p),
    ]


class TrackPositions(C.Structure):
    """``ctr_track_positions`` (include/ctrefine.h): the dense block of tracked clusters."""
    _fields_ = [
        ('ndim', C.c_int32), ('cluster_size', C.c_int32), ('n_frames', C.c_int64), ('n_features', C.c_int64),
        ('n_particles', C.c_int64), ('n_tracks', C.c_int64),
        ('frame_offset', C.c_void_p), ('particle', C.c_void_p), ('track_of_particle', C.c_void_p),
        ('pos', C.c_void_p), ('present', C.c_void_p), ('pos_out', C.c_void_p), ('status', C.c_void_p),
    ]


DRIFT_OK, DRIFT_BAD_TABLE = 0, 1                               # status[0] of the three drift calls


class Drift(C.Structure):
    """``ctr_drift`` (include/ctrefine.h): the drift of a linked video, frame by frame."""
    _fields_ = [
        ('ndim', C.c_int32), ('smoothing', C.c_int32),
        ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_particles', C.c_int64),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('particle', C.c_void_p),
        ('drift', C.c_void_p), ('n_pairs', C.c_void_p), ('status', C.c_void_p),
    ]


class DriftSubtract(C.Structure):
    """``ctr_drift_subtract`` (include/ctrefine.h): positions minus the drift of their frame."""
    _fields_ = [
        ('ndim', C.c_int32), ('reserved0', C.c_int32), ('n_frames', C.c_int64), ('n_features', C.c_int64),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('drift', C.c_void_p),
        ('pos_out', C.c_void_p), ('status', C.c_void_p),
    ]


class FilterStubs(C.Structure):
    """``ctr_filter_stubs`` (include/ctrefine.h): unlink the rows of short tracks."""
    _fields_ = [
        ('threshold', C.c_int64), ('n_features', C.c_int64), ('n_particles', C.c_int64),
        ('particle', C.c_void_p), ('particle_out', C.c_void_p), ('count', C.c_void_p), ('status', C.c_void_p),
    ]


MSD_OK, MSD_BAD_TABLE = 0, 1                                   # status[0] of ctr_msd_device and ctr_emsd_device
MSD_TILE, MSD_CHUNK = 2048, 256        # frames of a span dense in LDS; ids per partial of the ensemble


class Msd(C.Structure):
    """``ctr_msd`` (include/ctrefine.h): the mean squared displacement of every reported particle."""
    _fields_ = [
        ('ndim', C.c_int32), ('reserved0', C.c_int32), ('max_lagtime', C.c_int64),
        ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_particles', C.c_int64), ('n_select', C.c_int64),
        ('mpp', C.c_double * MAX_NDIM),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('particle', C.c_void_p), ('order', C.c_void_p),
        ('select', C.c_void_p),
        ('msd', C.c_void_p), ('mean_d', C.c_void_p), ('mean_d2', C.c_void_p), ('n', C.c_void_p), ('status', C.c_void_p),
    ]


class Emsd(C.Structure):
    """``ctr_emsd`` (include/ctrefine.h): the mean squared displacement of the ensemble."""
    _fields_ = [
        ('ndim', C.c_int32), ('reserved0', C.c_int32), ('max_lagtime', C.c_int64),
        ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_particles', C.c_int64),
        ('mpp', C.c_double * MAX_NDIM),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('particle', C.c_void_p), ('order', C.c_void_p),
        ('msd', C.c_void_p), ('mean_d', C.c_void_p), ('mean_d2', C.c_void_p), ('n', C.c_void_p), ('status', C.c_void_p),
    ]


VANHOVE_OK, VANHOVE_BAD_TABLE = 0, 1                           # status[0] of ctr_vanhove_device
VANHOVE_MAX_LAGS, VANHOVE_MAX_HALF_BINS = 64, 1024     # lags of a call; half the bins of a coordinate (counters in LDS)


class Vanhove(C.Structure):
    """``ctr_vanhove`` (include/ctrefine.h): the van Hove displacement distributions of the ensemble."""
    _fields_ = [
        ('ndim', C.c_int32), ('n_lags', C.c_int32), ('half_bins', C.c_int64),
        ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_particles', C.c_int64),
        ('bin_width', C.c_double), ('mpp', C.c_double * MAX_NDIM), ('lag', C.c_int64 * VANHOVE_MAX_LAGS),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('particle', C.c_void_p), ('order', C.c_void_p),
        ('edges', C.c_void_p), ('edge2', C.c_void_p),
        ('count', C.c_void_p), ('below', C.c_void_p), ('above', C.c_void_p), ('density', C.c_void_p),
        ('count_r', C.c_void_p), ('above_r', C.c_void_p), ('density_r', C.c_void_p), ('n', C.c_void_p),
        ('mean_d', C.c_void_p), ('mean_d2', C.c_void_p), ('mean_d4', C.c_void_p), ('alpha2', C.c_void_p),
        ('status', C.c_void_p),
    ]


PCF_OK, PCF_BAD_TABLE = 0, 1                                   # status[0] of ctr_pair_correlation_device
PCF_MAX_BINS = 2048                    # edge2 and the histogram of a workgroup are in LDS
PCF_EDGE_NONE, PCF_EDGE_INTERIOR, PCF_EDGE_ARC = 0, 1, 2       # ctr_pair_correlation.edge
PCF_EDGE_CODES = {'none': PCF_EDGE_NONE, 'interior': PCF_EDGE_INTERIOR, 'arc': PCF_EDGE_ARC}
PCF_PAIRS_ALL, PCF_PAIRS_SAME, PCF_PAIRS_OTHER = 0, 1, 2       # ctr_pair_correlation.pairs
PCF_PAIRS_CODES = {'all': PCF_PAIRS_ALL, 'same': PCF_PAIRS_SAME, 'other': PCF_PAIRS_OTHER}


class PairCorrelation(C.Structure):
    """``ctr_pair_correlation`` (include/ctrefine.h): the pair correlation function of a feature table."""
    _fields_ = [
        ('ndim', C.c_int32), ('edge', C.c_int32), ('pairs', C.c_int32), ('reserved0', C.c_int32),
        ('n_bins', C.c_int64), ('n_frames', C.c_int64), ('n_features', C.c_int64),
        ('dr', C.c_double), ('mpp', C.c_double * MAX_NDIM),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('group', C.c_void_p),
        ('box', C.c_void_p), ('edge2', C.c_void_p), ('shell', C.c_void_p),
        ('g', C.c_void_p), ('g_frame', C.c_void_p), ('count', C.c_void_p), ('weight', C.c_void_p),
        ('n_ref', C.c_void_p), ('n_rows', C.c_void_p), ('status', C.c_void_p),
    ]


NBR_OK, NBR_BAD_TABLE = 0, 1                                   # status[0] of ctr_neighbors_device
NBR_MAX_K = 16                         # the largest list a thread keeps in registers


class Neighbors(C.Structure):
    """``ctr_neighbors`` (include/ctrefine.h): nearest neighbours and proximity of a feature table;
    ``pairs`` takes the ``PCF_PAIRS_*`` codes."""
    _fields_ = [
        ('ndim', C.c_int32), ('pairs', C.c_int32), ('k', C.c_int32), ('lag', C.c_int32),
        ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_particles', C.c_int64),
        ('limit2', C.c_double), ('mpp', C.c_double * MAX_NDIM),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('group', C.c_void_p), ('particle', C.c_void_p),
        ('dist', C.c_void_p), ('dist2', C.c_void_p), ('index', C.c_void_p), ('count', C.c_void_p),
        ('particle_min', C.c_void_p), ('particle_min2', C.c_void_p), ('status', C.c_void_p),
    ]


TP_OK, TP_BAD_TABLE = 0, 1                                     # status[0] of ctr_twopoint_device
TP_MAX_BINS, TP_MAX_LAGS = 512, 16     # bins (edge2, counts and sums of a workgroup are in LDS); lags of a call
TP_MAX2_RANGE = (2. ** -500, 2. ** 500)                        # ctr_twopoint.max2: its square is finite, the unit 2^(e - 40) normal
TP_MAX_REACH2_MAX2 = 2. ** 1000                                # (n_bins dr)^2 max2 at most: no product of a pair overflows


class TwoPoint(C.Structure):
    """``ctr_twopoint`` (include/ctrefine.h): two-point displacement correlations of linked particles;
    ``pairs`` takes the ``PCF_PAIRS_*`` codes."""
    _fields_ = [
        ('ndim', C.c_int32), ('pairs', C.c_int32), ('n_lags', C.c_int32), ('reserved0', C.c_int32),
        ('n_bins', C.c_int64), ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_particles', C.c_int64),
        ('dr', C.c_double), ('max2', C.c_double), ('mpp', C.c_double * MAX_NDIM), ('lag', C.c_int64 * TP_MAX_LAGS),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('particle', C.c_void_p), ('group', C.c_void_p),
        ('edge2', C.c_void_p),
        ('n', C.c_void_p), ('dot', C.c_void_p), ('longitudinal', C.c_void_p), ('transverse', C.c_void_p), ('cos', C.c_void_p),
        ('sums', C.c_void_p), ('n_moved', C.c_void_p), ('beyond', C.c_void_p), ('status', C.c_void_p),
    ]


CON_COUNT, CON_FILL, CON_EPISODES = 0, 1, 2                   # ctr_contacts.phase
CON_OK, CON_BAD_TABLE, CON_OVERFLOW = 0, 1, 2                  # status[0] of ctr_contacts_device
CON_MAX_LIFETIME = 1 << 20                                     # ctr_contacts.max_lifetime at most


class Contacts(C.Structure):
    """``ctr_contacts`` (include/ctrefine.h): contact episodes and bond lifetimes of linked particles;
    ``pairs`` takes the ``PCF_PAIRS_*`` codes."""
    _fields_ = [
        ('phase', C.c_int32), ('ndim', C.c_int32), ('pairs', C.c_int32), ('reserved0', C.c_int32),
        ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_particles', C.c_int64), ('gap', C.c_int64),
        ('max_lifetime', C.c_int64), ('max_entries', C.c_int64),
        ('on2', C.c_double), ('off2', C.c_double), ('mpp', C.c_double * MAX_NDIM),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('particle', C.c_void_p), ('group', C.c_void_p),
        ('entry_start', C.c_void_p), ('n_entries', C.c_void_p), ('first_seen', C.c_void_p), ('last_seen', C.c_void_p),
        ('key', C.c_void_p), ('frame', C.c_void_p), ('d2', C.c_void_p),
        ('a', C.c_void_p), ('b', C.c_void_p), ('first', C.c_void_p), ('last', C.c_void_p), ('lifetime', C.c_void_p),
        ('n_seen', C.c_void_p), ('left_open', C.c_void_p), ('right_open', C.c_void_p), ('min_d2', C.c_void_p),
        ('max_d2', C.c_void_p),
        ('pair_a', C.c_void_p), ('pair_b', C.c_void_p), ('pair_episodes', C.c_void_p), ('pair_frames', C.c_void_p),
        ('pair_first', C.c_void_p), ('pair_last', C.c_void_p),
        ('formed', C.c_void_p), ('broken', C.c_void_p), ('active', C.c_void_p), ('lifetime_count', C.c_void_p),
        ('lifetime_above', C.c_void_p), ('duplicates', C.c_void_p), ('n_episodes', C.c_void_p), ('n_pairs', C.c_void_p),
        ('status', C.c_void_p),
    ]


SHAPE_MAX_COORDS, SHAPE_TILE, SHAPE_HALO_CAP = 19, 256, 768    # coordinates of a tetramer; the tiling of the dynamics
SHAPE_MAX_BOND_BINS, SHAPE_MAX_ANGLE_BINS = 4096, 1024         # counters of a workgroup in LDS


class Shape(C.Structure):
    """``ctr_shape`` (include/ctrefine.h): the shape coordinates of tracked clusters."""
    _fields_ = [
        ('ndim', C.c_int32), ('cluster_size', C.c_int32), ('n_tracks', C.c_int64), ('n_frames', C.c_int64),
        ('mpp', C.c_double * MAX_NDIM),
        ('pos', C.c_void_p), ('coords', C.c_void_p),
    ]


class ShapeDynamics(C.Structure):
    """``ctr_shape_dynamics`` (include/ctrefine.h): displacement statistics and static moments of the
    shape coordinates."""
    _fields_ = [
        ('ndim', C.c_int32), ('cluster_size', C.c_int32), ('n_tracks', C.c_int64), ('n_frames', C.c_int64),
        ('n_lags', C.c_int64), ('fps', C.c_double), ('mpp', C.c_double * MAX_NDIM),
        ('lags', C.c_void_p), ('pos', C.c_void_p),
        ('n', C.c_void_p), ('mean_d', C.c_void_p), ('mean_d2', C.c_void_p), ('mean_d4', C.c_void_p), ('flex', C.c_void_p),
        ('pooled_n', C.c_void_p), ('pooled_mean_d', C.c_void_p), ('pooled_mean_d2', C.c_void_p),
        ('pooled_mean_d4', C.c_void_p), ('pooled_flex', C.c_void_p),
        ('count', C.c_void_p), ('mean', C.c_void_p), ('var', C.c_void_p), ('min', C.c_void_p), ('max', C.c_void_p),
    ]


class ShapeHistogram(C.Structure):
    """``ctr_shape_histogram`` (include/ctrefine.h): the distributions of the shape coordinates."""
    _fields_ = [
        ('ndim', C.c_int32), ('cluster_size', C.c_int32), ('per_track', C.c_int32), ('reserved0', C.c_int32),
        ('n_tracks', C.c_int64), ('n_frames', C.c_int64), ('bond_bins', C.c_int64), ('angle_bins', C.c_int64),
        ('bond_dr', C.c_double), ('angle_width', C.c_double), ('mpp', C.c_double * MAX_NDIM),
        ('pos', C.c_void_p), ('bond_edges', C.c_void_p), ('angle_edges', C.c_void_p),
        ('count_bond', C.c_void_p), ('above', C.c_void_p), ('count_angle', C.c_void_p), ('n', C.c_void_p),
        ('density_bond', C.c_void_p), ('density_angle', C.c_void_p),
    ]


RESID_CHUNK = 256                                              # rows of a chunk of the frame pass
RESID_ZERO, RESID_NAN, RESID_IMAGE = 0, 1, 2                   # ctr_residual.outside
RESID_OK, RESID_BAD_TABLE, RESID_BAD_CLUSTER = 0, 1, 2         # ctr_residual.status[0]
INV_SERIES_MAX_PROFILE = 7                                     # profile parameters of inv_series_<N>: N + 1


class Residual(C.Structure):
    """``ctr_residual`` (include/ctrefine.h): model and residual frames of a fitted table."""
    _fields_ = [
        ('ndim', C.c_int32), ('frame_dtype', C.c_int32), ('fit_function', C.c_int32), ('isotropic', C.c_int32),
        ('n_profile', C.c_int32), ('outside', C.c_int32), ('want_frames', C.c_int32), ('want_model', C.c_int32),
        ('has_cluster', C.c_int32), ('max_grid', C.c_int32),
        ('n_frames', C.c_int64), ('n_features', C.c_int64),
        ('shape', C.c_int64 * MAX_NDIM), ('radius', C.c_int64 * MAX_NDIM),
        ('frames', C.c_void_p), ('frame_offset', C.c_void_p), ('params', C.c_void_p), ('mask_pos', C.c_void_p),
        ('cluster', C.c_void_p),
        ('residual', C.c_void_p), ('model', C.c_void_p), ('coverage', C.c_void_p), ('owner', C.c_void_p),
        ('n_pix', C.c_void_p), ('n_own', C.c_void_p), ('n_nan', C.c_void_p), ('sum', C.c_void_p), ('sum_sq', C.c_void_p),
        ('own_sum_sq', C.c_void_p), ('max_abs', C.c_void_p), ('rms', C.c_void_p),
        ('cluster_n_pix', C.c_void_p), ('cluster_sum_sq', C.c_void_p), ('cost', C.c_void_p),
        ('status', C.c_void_p),
    ]


FITERR_OK, FITERR_NOT_POSITIVE_DEFINITE, FITERR_NONFINITE, FITERR_EMPTY, FITERR_TOO_LARGE, FITERR_BAD_TABLE = range(6)   # ctr_fit_error.status
FITERR_MAX_ROWS = 64                                           # rows of a cluster of ctr_fit_error_device
FITERR_CLASSES = 3                                             # size classes of its launches


class FitError(C.Structure):
    """``ctr_fit_error`` (include/ctrefine.h): standard errors and covariance of a fitted table."""
    _fields_ = [
        ('ndim', C.c_int32), ('frame_dtype', C.c_int32), ('fit_function', C.c_int32), ('isotropic', C.c_int32),
        ('n_profile', C.c_int32), ('want_cov', C.c_int32), ('max_grid', C.c_int32), ('reserved0', C.c_int32),
        ('modes', C.c_int32 * MAX_PARAMS),
        ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_clusters', C.c_int64),
        ('n_vars_total', C.c_int64), ('n_cov_total', C.c_int64),
        ('shape', C.c_int64 * MAX_NDIM), ('radius', C.c_int64 * MAX_NDIM),
        ('residual_factor', C.c_double),
        ('frames', C.c_void_p), ('frame_offset', C.c_void_p), ('params', C.c_void_p), ('mask_pos', C.c_void_p),
        ('order', C.c_void_p), ('cluster_offset', C.c_void_p), ('var_offset', C.c_void_p), ('cov_offset', C.c_void_p),
        ('params_std', C.c_void_p), ('status', C.c_void_p), ('n_vars', C.c_void_p), ('n_pix', C.c_void_p),
        ('cov', C.c_void_p), ('var_row', C.c_void_p), ('var_col', C.c_void_p),
    ]


PREPARE_BATCH, PREPARE_SCATTER = 0, 1                         # ctr_refine_prepare.mode
PREPARE_OK, PREPARE_BAD_TABLE, PREPARE_INFEASIBLE = 0, 1, 2    # ctr_refine_prepare.status[0]


class RefinePrepare(C.Structure):
    """``ctr_refine_prepare`` (include/ctrefine.h): a refine batch from device tables, and the
    scatter of its results into input row order."""
    _fields_ = [
        ('mode', C.c_int32), ('ndim', C.c_int32), ('n_params', C.c_int32), ('reserved0', C.c_int32),
        ('modes', C.c_int32 * MAX_PARAMS),
        ('n_frames', C.c_int64), ('n_features', C.c_int64), ('n_clusters', C.c_int64),
        ('separation', C.c_double * MAX_NDIM),
        ('bound_abs', C.c_double * (2 * MAX_PARAMS)), ('bound_diff', C.c_double * (2 * MAX_PARAMS)),
        ('bound_rel', C.c_double * (2 * MAX_PARAMS)),
        ('pos', C.c_void_p), ('frame_offset', C.c_void_p), ('params0', C.c_void_p),
        ('label', C.c_void_p), ('cluster_size', C.c_void_p), ('order', C.c_void_p),
        ('feat_offset', C.c_void_p), ('frame_index', C.c_void_p), ('n_clusters_out', C.c_void_p),
        ('params', C.c_void_p), ('low', C.c_void_p), ('high', C.c_void_p), ('status', C.c_void_p),
        ('fit_params', C.c_void_p), ('fit_cost', C.c_void_p), ('fit_std', C.c_void_p),
        ('params_out', C.c_void_p), ('cost_out', C.c_void_p), ('std_out', C.c_void_p),
    ]


class Orientation(C.Structure):
    """``ctr_orientation`` (include/ctrefine.h): orientation of tracked clusters on the device."""
    _fields_ = [
        ('ndim', C.c_int32), ('cluster_size', C.c_int32), ('n_tracks', C.c_int64),
        ('n_frames', C.c_int64), ('mpp', C.c_double), ('weights', C.c_double * 4),
        ('pos', C.c_void_p), ('angles', C.c_void_p), ('com', C.c_void_p), ('bases', C.c_void_p),
    ]


class Diffusion(C.Structure):
    """``ctr_diffusion`` (include/ctrefine.h): diffusion tensor of tracked clusters on the device."""
    _fields_ = [
        ('ndim', C.c_int32), ('n_perm', C.c_int32), ('n_tracks', C.c_int64),
        ('n_frames', C.c_int64), ('n_lags', C.c_int64), ('fps', C.c_double),
        ('lags', C.c_void_p), ('positions', C.c_void_p), ('bases', C.c_void_p),
        ('tensor', C.c_void_p), ('n_samples', C.c_void_p),
    ]


CI_BCA, CI_PI = 0, 1                                           # ctr_diffusion_ci.method
DIFFUSION_CI_MAX_SAMPLES, DIFFUSION_CI_MAX_ALPHA = 16384, 8
DIFFUSION_CI_LDS_BYTES, DIFFUSION_CI_SCRATCH_BYTES = 65536, 268435456


class DiffusionCI(C.Structure):
    """``ctr_diffusion_ci`` (include/ctrefine.h): bootstrap interval of the diffusion tensor on the device."""
    _fields_ = [
        ('ndim', C.c_int32), ('n_perm', C.c_int32), ('n_tracks', C.c_int64),
        ('n_frames', C.c_int64), ('n_lags', C.c_int64), ('fps', C.c_double),
        ('lags', C.c_void_p), ('positions', C.c_void_p), ('bases', C.c_void_p),
        ('n_samples', C.c_int64), ('seed', C.c_uint64), ('method', C.c_int32), ('n_alpha', C.c_int32),
        ('z_alpha', C.c_double * DIFFUSION_CI_MAX_ALPHA), ('alphas', C.c_double * DIFFUSION_CI_MAX_ALPHA),
        ('pool_tracks', C.c_int32),
        ('interval', C.c_void_p), ('tensor', C.c_void_p), ('n_rows', C.c_void_p),
        ('z0', C.c_void_p), ('accel', C.c_void_p), ('ranks', C.c_void_p),
    ]


def make_problem(ndim, isotropic, modes, radius, constraint=None, max_iter=10,
                 max_shift=1., max_rms_dev=1., residual_factor=100000.,
                 solver_maxiter=100, xtol=0., ftol=0., noise_size=None, threshold=None,
                 fit_function='gauss'):
    """Fill a ``ctr_problem``.  ``constraint`` = None or (kind, dist[ndim]); ``noise_size`` = None
    or one sigma per axis (refine.py:37-40)."""
    p = Problem()
    p.ndim = int(ndim)
    p.isotropic = int(bool(isotropic))
    p.fit_function, n_extra = fit_code(fit_function)
    p.n_params = 2 + ndim + (1 if isotropic else ndim) + n_extra
    if p.n_params > MAX_PARAMS:
        raise NotImplementedError("%s in %dD%s: %d parameter columns, the engine takes %d"
                                  % (fit_function, ndim, '' if isotropic else ' anisotropic', p.n_params, MAX_PARAMS))
    if len(modes) != p.n_params:
        raise ValueError("modes must have %d entries" % p.n_params)
    for i, m in enumerate(modes):
        p.modes[i] = int(m)
    for i, r in enumerate(radius):
        p.radius[i] = int(r)
    if constraint is not None:
        kind, dist = constraint
        p.constraint_kind = CONS_CODES[kind]
        for i, d in enumerate(dist):
            p.constraint_dist[i] = float(d)
    p.max_iter = int(max_iter)
    p.solver_maxiter = int(solver_maxiter)
    p.max_shift = float(max_shift)
    p.max_rms_dev = float(max_rms_dev)
    p.residual_factor = float(residual_factor)
    p.xtol = float(xtol)
    p.ftol = float(ftol)
    if noise_size is not None:
        for i, sgm in enumerate(noise_size):
            if not (0 <= float(sgm) <= MAX_NOISE_SIZE):
                raise ValueError("noise_size must be between 0 and %g" % MAX_NOISE_SIZE)
            p.noise_size[i] = float(sgm)
        p.threshold = 0. if threshold is None else float(threshold)   # refine.py:38-39
        p.flags |= FLAG_WINDOW_FILTER                                 # refine.py:37: `is not None`
    return p


class HostBatch(object):
    """NumPy-owned buffers of one batch + the ``ctr_batch`` view onto them."""

    def __init__(self, frames, frame_index, feat_offset, params, low, high, want_std=False):
        frames = np.asarray(frames)
        if frames.dtype not in DTYPE_CODES:
            # every other pixel type is widened to f64 exactly like
            # ``.astype(np.float64)`` in the reference (refine.py:58)
            frames = frames.astype(np.float64)
        self.frames = np.ascontiguousarray(frames)
        self.frame_index = np.ascontiguousarray(frame_index, dtype=np.int32)
        self.feat_offset = np.ascontiguousarray(feat_offset, dtype=np.int32)
        self.params = np.ascontiguousarray(params, dtype=np.float64)
        self.low = np.ascontiguousarray(low, dtype=np.float64)
        self.high = np.ascontiguousarray(high, dtype=np.float64)
        n_cl = len(self.frame_index)
        if len(self.feat_offset) != n_cl + 1:
            raise ValueError("feat_offset must have n_clusters + 1 entries")
        n_feat = int(self.feat_offset[-1]) if n_cl else 0
        if self.params.ndim != 2 or self.params.shape[0] != n_feat:
            raise ValueError("params must be [n_features, n_params]")
        if self.low.shape != self.params.shape or self.high.shape != self.params.shape:
            raise ValueError("low/high must match params")
        if n_cl and (self.frame_index.min() < 0 or
                     self.frame_index.max() >= self.frames.shape[0]):
            raise ValueError("frame_index out of range")
        if n_cl and np.any(np.diff(self.feat_offset) < 0):
            raise ValueError("feat_offset must be non-decreasing")
        self.params_out = np.empty_like(self.params)
        self.cost = np.full(n_cl, np.nan)
        self.status = np.zeros(n_cl, dtype=np.int32)
        self.n_rounds = np.zeros(n_cl, dtype=np.int32)
        self.n_iter = np.zeros(n_cl, dtype=np.int32)
        # refine.py:400-406 (compute_error): one standard deviation per fitted parameter
        self.params_std = np.full_like(self.params, np.nan) if want_std else None

    @property
    def n_clusters(self):
        return len(self.frame_index)

    @property
    def n_features(self):
        return self.params.shape[0]

    def as_struct(self):
        b = Batch()
        b.frames = self.frames.ctypes.data
        b.frame_dtype = DTYPE_CODES[self.frames.dtype]
        b.n_frames = self.frames.shape[0]
        for i, s in enumerate(self.frames.shape[1:]):
            b.shape[i] = int(s)
        b.n_clusters = self.n_clusters
        b.n_features = self.n_features
        for name in ('frame_index', 'feat_offset', 'params', 'low', 'high',
                     'params_out', 'cost', 'status', 'n_rounds', 'n_iter'):
            setattr(b, name, getattr(self, name).ctypes.data)
        b.params_std = self.params_std.ctypes.data if self.params_std is not None else None
        return b
