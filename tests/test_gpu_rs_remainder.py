"""On the device: the Reed-Solomon syndromes from the generator-polynomial remainder (k_rs_superframes through dabphy_rs_superframes) and
the superframe filter's wide pass with several attempts per work-group (k_superframe_wide through streams), against the oracle, no tolerance.
The cases are those of tests/test_emu_rs_remainder.py (tests/rs_remainder_cases.py)."""
import pytest

import rs_remainder_cases as C
from conftest import GPU_LIB

pytestmark = pytest.mark.gpu


def factory(**kw):
    from welle_io_amd import capi
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


@pytest.mark.parametrize("s", C.RS_S)
def test_syndromes_from_the_remainder(gpu, s):
    C.check_rs_syndromes(gpu, s)


@pytest.mark.parametrize("name", sorted(C.WIDE_CASES))
def test_wide_pass_attempts_per_work_group(gpu, name):
    C.check_wide_groups(factory, name)


def test_wide_pass_other_buckets(gpu):
    C.check_wide_other_buckets(factory)


def test_wide_pass_layouts(gpu):
    C.check_wide_layouts(factory)


def test_wide_pass_timing_driver(gpu):
    C.check_wide_timing_driver(factory)
