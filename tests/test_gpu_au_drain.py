"""GPU suite: the bulk access-unit drain (dabphy_set_au_drain / dabphy_au_drain_*, k_au.hip) on the device against tests/au_model.py on
the oracle's filter events -- the cases of tests/au_cases.py: the unit sweep through dabphy_test_au_pack, the whole cross of batch depth,
filter mode and format through the stream, MP2 beside DAB+, different lists, a list change behind a deferred pass, a replayed batch, the
begin / wait protocol beside an MSC drain."""
import pytest

import au_cases as A
from conftest import GPU_LIB
from welle_io_amd import capi

pytestmark = pytest.mark.gpu


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_unit_corners(gpu, fmt):
    A.check_unit_corners(gpu, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_unit_length_and_alignment_sweep(gpu, fmt):
    A.check_unit_sweep(gpu, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_unit_capacity(gpu, fmt):
    A.check_unit_capacity(gpu, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("F", [3, 5])
def test_through_the_stream(gpu, F, mode, fmt):
    A.check_stream(factory, F, mode, fmt)


def test_manual_filter_pass(gpu):
    A.check_stream(factory, 3, 0, capi.AU_LOAS)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_mp2_beside_dabplus(gpu, fmt):
    A.check_mp2_beside_dabplus(factory, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_two_ensembles_with_different_lists(gpu, fmt):
    A.check_two_lists(factory, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_list_change_behind_a_deferred_pass(gpu, fmt):
    A.check_list_change(factory, fmt)


@pytest.mark.parametrize("fmt", A.FORMATS)
@pytest.mark.parametrize("mode", [1, 2])
def test_behind_a_replayed_batch(gpu, fmt, mode):
    A.check_replay(factory, fmt, mode)


@pytest.mark.parametrize("fmt", A.FORMATS)
@pytest.mark.parametrize("mode", [1, 2])
def test_replayed_batch_that_stores_access_units(gpu, fmt, mode):
    A.check_replay_storing(factory, fmt, mode)


@pytest.mark.parametrize("fmt", A.FORMATS)
def test_protocol(gpu, fmt):
    A.check_protocol(factory, fmt)
