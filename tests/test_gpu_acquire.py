"""GPU suite: the acquisition head of the synchroniser on the device -- acquire_body, slevel_replay and k_slevel_catchup of k_sync.hip, case by
case through the public streaming calls on the directed streams of tests/acquire_cases.py, against the restatement's attempt trace: window
search positions, indices and correctors as exact integers, impulse responses bit for bit, notSynced counts."""
import pytest

import acquire_cases as A
from conftest import GPU_LIB
from welle_io_amd import capi

pytestmark = pytest.mark.gpu


def factory(**kw):
    return capi.DabPhy(lib_path=GPU_LIB, **kw)


@pytest.mark.parametrize("feed", A.FEEDS)
@pytest.mark.parametrize("name", A.FAMILIES[:-1])
def test_acquire_family(gpu, name, feed):
    A.check_family(factory, name, feed)


@pytest.mark.parametrize("mode", ["oneshot", "frames", "track_slevel", "pipeline_sync_3"])
def test_reacquire_with_the_oscillator_running(gpu, mode):
    if mode == "pipeline_sync_3":
        A.check_family(factory, "reacquire", "oneshot", pipeline_sync=3)
    else:
        A.check_family(factory, "reacquire", "oneshot" if mode == "track_slevel" else mode, track_slevel=mode == "track_slevel")
