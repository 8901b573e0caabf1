"""GPU-less logic check of the Reed-Solomon syndromes from the generator-polynomial remainder and of the superframe filter's wide pass
with several attempts per work-group: the kernel sources on the CPU execution model of tests/hipemu against the oracle, no tolerance.
(tests/test_gpu_rs_remainder.py runs the same cases on the device.)"""
import pytest

import rs_remainder_cases as C


def factory(**kw):
    from welle_io_amd import capi
    import conftest
    return capi.DabPhy(lib_path=conftest.EMU_LIB, **kw)


@pytest.mark.parametrize("s", C.RS_S)
def test_syndromes_from_the_remainder(emu, s):
    """a single error at each of the 120 positions, five and six errors through the same places, clean / zero / 0xFF words and the directed
    corner words, neighbours in the lanes, at 1, 8, 9 and 48 code words per superframe: bytes, counts and verdicts are the oracle's"""
    C.check_rs_syndromes(emu, s)


@pytest.mark.parametrize("name", sorted(C.WIDE_CASES))
def test_wide_pass_attempts_per_work_group(emu, name):
    """a pair's attempts per batch one, seven, eight and nine (64 kbit/s: eight to a work-group), 0 .. 4 frames carried, the lost superframe
    in the first and in the last attempt of a work-group and alone in a second one: events, superframes and totals are the oracle's, and both
    the settled and the walked way through a batch were taken"""
    C.check_wide_groups(factory, name)


def test_wide_pass_other_buckets(emu):
    C.check_wide_other_buckets(factory)


def test_wide_pass_layouts(emu):
    C.check_wide_layouts(factory)


def test_wide_pass_timing_driver(emu):
    C.check_wide_timing_driver(factory)
