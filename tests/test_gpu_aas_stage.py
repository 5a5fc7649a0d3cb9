"""GPU: data services as the gfx950 code computes them -- k_aas over a packet arena in device memory, only the events copied back -- through
nrsc5hip_stage_aas on the packet lists of tests/aas_args.py, against the model of tests/aas_model.py (event for event, counter for counter, SIG snapshot
for snapshot: tests/aas_checks.py); chained behind k_psd through nrsc5hip_stage_aas_frames, with the byte bound and a carousel sent three times; and end
to end through nrsc5hip_aas_feed against the unmodified reference's public-API events.  The same checks run on the emulated build in
tests/test_aas_stage_cpu.py, which also holds the tests of the lists and of the model.  A list is at most 260 packets; a chain a few short frames."""
import pytest

from tests import aas_args as aa, aas_checks as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E(hip_lib):
    e = ac.make_engine(hip_lib)
    yield e
    e.close()


@pytest.mark.parametrize("name", aa.NAMES)
def test_gpu_list_in_one_call_equals_the_model(E, name):
    ac.check_list_in_one_call(E, name)


@pytest.mark.parametrize("name", ("files", "headers", "changes", "lru", "pool", "aligned", "signone"))
def test_gpu_one_packet_per_call_equals_the_model(E, name):
    ac.check_packet_per_call(E, name)


def test_gpu_fragment_events_only_with_the_flag(E):
    ac.check_fragment_flag_off(E)


def test_gpu_three_consumer_streams_in_one_call(E):
    ac.check_three_streams_in_one_call(E)


def test_gpu_reset_between_two_lists(E):
    ac.check_reset(E)


def test_gpu_arena_overflow_is_reported(E):
    ac.check_arena_overflow(E)


def test_gpu_rejections_leave_state_and_counters_untouched(hip_lib):
    ac.check_rejections(hip_lib)


def test_gpu_chain_behind_k_psd_three_streams(E):
    ac.check_chain(E)


def test_gpu_carousel_sent_three_times_moves_the_files_once(E):
    ac.check_carousel(E)


def test_gpu_end_to_end_feed_equals_the_reference(hip_lib, reflib):
    ac.check_feed_end_to_end(hip_lib, reflib)
