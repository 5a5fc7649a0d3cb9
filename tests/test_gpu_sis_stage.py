"""GPU: SIS as the gfx950 code computes it -- k_sis over packed PIDS frames, only the events copied back -- through nrsc5hip_stage_sis on the frame sets of
tests/sis_args.py, against the model of tests/sis_model.py (event for event, counter for counter, snapshot for snapshot: tests/sis_checks.py), and end to
end through nrsc5hip_sis_feed against the unmodified reference's public-API events.  The same checks run on the emulated build in
tests/test_sis_stage_cpu.py, which also holds the tests of the sets and of the model.  A set is at most 256 frames of 80 bits."""
import pytest

from tests import sis_args as sa, sis_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E(hip_lib):
    e = sc.make_engine(hip_lib)
    yield e
    e.close()


@pytest.mark.parametrize("name", sa.NAMES)
def test_gpu_set_in_one_call_equals_the_model(E, name):
    sc.check_set_in_one_call(E, name)


@pytest.mark.parametrize("name", ("schedule", "random1", "am"))
def test_gpu_one_frame_per_call_equals_the_model(E, name):
    sc.check_pieces(E, name, 1)


@pytest.mark.parametrize("piece", (63, 64, 65, 129))
def test_gpu_pieces_around_the_chunk_boundary(E, piece):
    for name in ("random3", "random4"):
        sc.check_pieces(E, name, piece)


def test_gpu_rewritten_lengths_of_displayed_items_stay_inside_the_snapshot(E):
    sc.check_rewritten_lengths(E)


def test_gpu_three_consumer_streams_in_one_call(E):
    sc.check_three_streams_in_one_call(E)


def test_gpu_reset_in_front_of_a_frame_mid_item_and_behind_the_last(E):
    sc.check_reset_at(E)


def test_gpu_sis_reset_mid_item(E):
    sc.check_reset_mid_item(E)


def test_gpu_arena_overflow_is_reported(E):
    sc.check_arena_overflow(E)


def test_gpu_rejections_leave_state_and_counters_untouched(hip_lib):
    sc.check_rejections(hip_lib)


def test_gpu_end_to_end_feed_in_record_pieces_equals_the_reference(hip_lib, reflib):
    sc.check_feed_end_to_end(hip_lib, reflib)
