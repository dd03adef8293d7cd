"""The one path from a stage descriptor to its launch: the signature table of
``_lib`` against the header, the order descriptor / handle of every entry point that goes through
``run_stage``, and a library without the symbols.  No device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.special import ndtri

import _cases
from clustertracking_amd import _abi, _lib, relocate


def test_argtypes_count_matches_the_header():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', header))
    assert set(protos) == set(_lib.SIGNATURES) and _lib.EXPORTS == tuple(_lib.SIGNATURES)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        params = protos[name].strip()
        n = 0 if params in ('', 'void') else len(params.split(','))
        assert len(argtypes) == n, (name, params)


def _characterize():
    d = _abi.Characterize()
    d.ndim, d.frame_dtype, d.n_frames = 2, _abi.DTYPE_CODES[np.dtype(np.uint8)], 1
    d.shape[0] = d.shape[1] = 16
    d.radius[0] = d.radius[1] = 3
    d.isotropic, d.scale_factor, d.n_features = 1, 1., 0
    d.pos = 8          # never read: there is no feature
    return d


def _preprocess():
    d = _abi.Preprocess()
    d.ndim, d.frame_dtype, d.n_frames = 2, 0, 1
    d.shape[0], d.shape[1] = 32, 40
    d.mode, d.strategy = _abi.PRE_PREPROCESS, _abi.PRE_AUTO
    for a in range(2):
        d.n_taps[a], d.box[a], d.taps[a] = 9, 13, 64
    d.threshold = 1.
    d.frames = d.out = d.scale_factor = 64     # never dereferenced: there is no handle
    return d


def _link():
    d = _abi.Link()
    d.ndim, d.memory, d.n_levels, d.n_features = 2, 0, 3, 0
    d.search_range[0] = d.search_range[1] = 5.
    return d


def _orientation():
    d = _abi.Orientation()
    d.ndim, d.cluster_size, d.n_tracks, d.n_frames, d.mpp = 2, 2, 0, 0, 1.
    d.weights[0] = d.weights[1] = 1.
    return d


def _diffusion():
    d = _abi.Diffusion()
    d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = 2, 2, 0, 0, 0, 1.
    return d


def _diffusion_ci():
    d = _abi.DiffusionCI()
    d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = 2, 2, 0, 0, 0, 1.
    d.n_samples, d.method, d.n_alpha = 1, _abi.CI_PI, 1
    d.alphas[0], d.z_alpha[0] = 0.5, ndtri(0.5)
    return d


def _relocate():
    return relocate.descriptor((48, 56), np.uint8, 1, 9, 11, 5)      # no query


STAGES = [('ctr_characterize_device', _characterize), ('ctr_preprocess_device', _preprocess),
          ('ctr_link_device', _link), ('ctr_orientation_device', _orientation),
          ('ctr_diffusion_device', _diffusion), ('ctr_diffusion_ci_device', _diffusion_ci),
          ('ctr_relocate_device', _relocate)]


@pytest.mark.parametrize('call,descriptor', STAGES, ids=[s[0] for s in STAGES])
def test_descriptor_then_handle(call, descriptor):
    """with a NULL handle: no descriptor is refused as such, a valid one reaches "null handle";
    both under the entry point's name"""
    lib = _lib.load()
    fn = getattr(lib, call)
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    assert fn(None, None, None) == _abi.ERR_INVALID
    assert msg().startswith(call + ': ') and msg() != call + ': null handle'
    assert fn(None, ctypes.byref(descriptor()), None) == _abi.ERR_INVALID
    assert msg() == call + ': null handle'


def test_library_without_the_symbols_is_refused(tmp_path):
    src = tmp_path / 'stub.c'
    src.write_text('int ctr_abi_version(void) {\n  return %d;\n}\n' % _abi.ABI_VERSION)
    so = tmp_path / 'libstub.so'
    subprocess.check_call(['gcc', '-shared', '-fPIC', str(src), '-o', str(so)])
    code = ("from clustertracking_amd import _lib\n"
            "try:\n    _lib.load()\nexcept _lib.EngineError as e:\n    print('REFUSED', e)\n")
    env = dict(os.environ, CTREFINE_LIB=str(so),
               PYTHONPATH=os.pathsep.join(filter(None, [_cases.ROOT, os.environ.get('PYTHONPATH')])))
    out = subprocess.run([sys.executable, '-c', code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=120).stdout
    assert 'REFUSED' in out and 'ctr_create' in out and 'ctr_link_device' in out and 'rebuild' in out, out
    assert 'ctr_abi_version,' not in out
