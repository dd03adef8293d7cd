"""clustertracking_amd -- MI355X-native engine for the per-cluster least-squares
refinement of caspervdw/clustertracking (``refine_leastsq``).

Public names follow the reference package (``clustertracking/__init__.py:10-18``)
for the part of it that this engine accelerates.
"""
import logging

from .refine import refine_leastsq, refine_arrays, prepare_batch, write_back
from .find import (find_clusters, grey_dilation, locate_maxima, percentile_threshold,
                   where_close, drop_close, characterize, characterize_arrays, locate)
from .preprocessing import lowpass, bandpass, preprocess
from .relocate import relocate_arrays, relocate_candidates
from .find_link import find_link, find_link_arrays
from .refine_com import refine_com, refine_com_arrays
from .train import train_leastsq, train_arrays
from .refine_global import refine_global_arrays, refine_global   # the function shadows the submodule, as vanhove does
from .fitfunc import FitFunctions
from .utils import ArrayReader, RefineException
from . import constraints, artificial, link, motion, motion_ci, preprocessing
from .motion_ci import diffusion_tensor_ci, bootstrap_indices
from .cluster_tracks import cluster_tracks, cluster_tracks_arrays, track_positions, track_positions_arrays
from . import drift
from .drift import (compute_drift, subtract_drift, filter_stubs, compute_drift_arrays, subtract_drift_arrays,
                    filter_stubs_arrays)
from . import msd
from .msd import msd_arrays, emsd_arrays, imsd, emsd
from .vanhove import vanhove_arrays, vanhove     # the function shadows the submodule: importlib.import_module reaches it
from . import static
from .static import pair_correlation_arrays, pair_correlation, neighbors_arrays, neighbors, proximity
from .twopoint import twopoint_arrays, twopoint   # the function shadows the submodule, as vanhove does
from . import shape
from .shape import (shape_arrays, shape_dynamics_arrays, shape_histogram_arrays, shape_names, shape_df, flexibility)
from .residual import residual_arrays, residual   # the function shadows the submodule, as vanhove does
from .contacts import contacts_arrays, contacts, bonds, contact_lifetimes   # the function shadows the submodule, as vanhove does
from .fit_error import fit_error_arrays, fit_error   # the function shadows the submodule and carries distance_std

link_df = link.link
link_arrays = link.link_arrays

__all__ = ['refine_leastsq', 'refine_arrays', 'train_leastsq', 'train_arrays', 'refine_global', 'refine_global_arrays', 'find_clusters', 'grey_dilation', 'locate_maxima',
           'characterize', 'characterize_arrays', 'locate', 'relocate_arrays', 'relocate_candidates', 'find_link', 'find_link_arrays', 'refine_com', 'refine_com_arrays', 'lowpass', 'bandpass', 'preprocess', 'preprocessing',
           'percentile_threshold', 'where_close', 'drop_close', 'link', 'link_df', 'link_arrays', 'FitFunctions', 'constraints',
           'artificial', 'ArrayReader', 'RefineException', 'prepare_batch',
           'write_back', 'motion', 'motion_ci', 'diffusion_tensor_ci', 'bootstrap_indices',
           'cluster_tracks', 'cluster_tracks_arrays', 'track_positions', 'track_positions_arrays',
           'drift', 'compute_drift', 'subtract_drift', 'filter_stubs', 'compute_drift_arrays', 'subtract_drift_arrays',
           'filter_stubs_arrays', 'msd', 'msd_arrays', 'emsd_arrays', 'imsd', 'emsd',
           'vanhove_arrays', 'vanhove', 'static', 'pair_correlation_arrays', 'pair_correlation',
           'neighbors_arrays', 'neighbors', 'proximity', 'twopoint_arrays', 'twopoint',
           'shape', 'shape_arrays', 'shape_dynamics_arrays', 'shape_histogram_arrays', 'shape_names', 'shape_df',
           'flexibility', 'residual_arrays', 'residual', 'contacts_arrays', 'contacts', 'bonds', 'contact_lifetimes',
           'fit_error_arrays', 'fit_error']

logger = logging.getLogger(__name__)
logger.addHandler(logging.NullHandler())
