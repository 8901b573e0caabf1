"""CPU suite: the acquisition head of the synchroniser (acquire_body, slevel_replay, k_slevel_catchup of k_sync.hip) on the execution model
of tests/hipemu, case by case through the public streaming calls on the directed streams of tests/acquire_cases.py, against the
restatement's attempt trace -- which tests/test_oracle_vs_ref.py pins to the reference on the same streams.  tests/test_gpu_acquire.py
runs the same cases on the device."""
import pytest

import acquire_cases as A
from conftest import EMU_LIB
from welle_io_amd import capi


def factory(**kw):
    return capi.DabPhy(lib_path=EMU_LIB, **kw)


def test_case_set_reaches_its_branches():
    """from the restatement's traces alone: no device, nothing the code under test could satisfy"""
    A.validate()


@pytest.mark.parametrize("feed", A.FEEDS)
@pytest.mark.parametrize("name", A.FAMILIES[:-1])
def test_acquire_family(emu, name, feed):
    A.check_family(factory, name, feed)


@pytest.mark.parametrize("mode", ["oneshot", "frames", "track_slevel"])
def test_reacquire_with_the_oscillator_running(emu, mode):
    A.check_family(factory, "reacquire", "oneshot" if mode == "track_slevel" else mode, track_slevel=mode == "track_slevel")
