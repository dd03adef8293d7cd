"""No kernel of the global fit (csrc/global_kernels.h) uses scratch memory: what the compiler
recorded in the gfx950 code object of the built library, for every instantiation (CPU only)."""
import re

import pytest

import _resources


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    try:
        out = _resources.metadata('global_', tmp_path_factory.mktemp('co'))
    except _resources.Unavailable as e:
        pytest.skip(str(e))
    return {k: v for k, v in out.items() if re.search(r'global_(eval|judge|factor|solve|setup)_kernel', k)}


def test_every_instantiation_is_there(kernels):
    evals = [k for k in kernels if 'global_eval_kernel' in k]
    assert len(evals) == 2 * 2 * 4 * 3      # ND, ISO, FIT, NT
    assert len(kernels) == len(evals) + 4


def test_no_kernel_has_scratch(kernels):
    bad = {k: v['.private_segment_fixed_size'] for k, v in kernels.items() if int(v['.private_segment_fixed_size']) != 0}
    assert not bad, 'scratch bytes per lane: %s' % bad
    assert not [k for k, v in kernels.items() if int(v.get('.vgpr_spill_count', 0)) != 0]
