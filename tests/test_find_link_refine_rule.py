"""``find_link(refine=True)``, the rule: the yardstick loop of
tests/_find_link_refine.py against the reference's tables of
tests/golden/find_link/find_link_refine_cases.npz (the reference's ``_find_link_iter`` with the
refinement as its ``after_link`` callback).  No device."""
import numpy as np
import pytest

import _find_link as F
import _find_link_refine as R

FIXTURES = R.fixtures()


def test_fixtures_are_the_four_cases():
    assert [f[0] for f in FIXTURES] == ['2d_iso_u8_m0', '2d_iso_u16_m1', '2d_iso_f64_m2', '3d_aniso_u8_m0']
    assert [f[1].dtype.name for f in FIXTURES] == ['uint8', 'uint16', 'float64', 'uint8']
    assert [f[2]['memory'] for f in FIXTURES] == [0, 1, 2, 0] and FIXTURES[1][2]['scale_factor'] == 2.
    assert FIXTURES[3][1].ndim == 4
    z = np.load(R.GOLDEN)
    n_walked = sum(int((z['n_iter_%d' % i] >= 2).sum()) for i in range(4))
    n_clipped = sum(int(z['clipped_%d' % i].sum()) for i in range(4))
    assert n_walked >= 10 and n_clipped >= 1
    assert all(int(z['relocated_%d' % i].sum()) >= 3 for i in range(4))
    # the refinement moved the rows: the fixtures are not those of find_link_cases.npz
    assert all(np.any(z['pos_%d' % i] != z['start_%d' % i]) for i in range(4))


@pytest.mark.parametrize('index', range(len(FIXTURES)), ids=[f[0] for f in FIXTURES])
def test_yardstick_equals_the_reference(index):
    """particle, frame and relocated exactly; positions and mass bit for bit on the integer cases
    and to 1e-10 / rtol 1e-12 on float64"""
    name, frames, kw, want = FIXTURES[index]
    got = R.find_link(frames, **kw)
    R.assert_equals_fixture(got, want, frames.ndim - 1, F.is_isotropic(kw), exact=frames.dtype.kind in 'ui')
    z = np.load(R.GOLDEN)
    o = F.sorted_rows(got, frames.ndim - 1)
    assert np.array_equal(got['n_iter'][o], z['n_iter_%d' % index])
    assert np.array_equal(got['start'][o], z['start_%d' % index])
