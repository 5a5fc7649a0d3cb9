"""`-m "not gpu"`: the coarse-acquisition stage hooks on the CPU-emulated twin -- the production kernels' indexing (list walk, history, sliding
sum, arg-max and its tie-break), their tables (engine.hip: build_tables -> acq_q15, am_acq_q15, shape, am_shape) and the hooks' bookkeeping against
the oracle's twins, bit for bit, on the inputs of tests/acq_args.py (tests/acq_checks.py says what is compared and why the end-to-end tests cannot
see it).  What only the device can show -- the generated code of the same kernels, the wave reductions in hardware -- is
tests/test_gpu_acquire_stage.py's, which runs the same checks.  Also here: the argument checks of the hooks, and what the input sets hold."""
import pytest

from tests import acq_args as aa, acq_checks as ac

# The emulated build runs the list test with all LIST_N = 95 streams (65 active), as the device does: about a second here.
LIST_N_EMU = aa.LIST_N


@pytest.fixture(scope="module")
def fifo(emu_lib):
    e = ac.make_engine(emu_lib, "fifo", aa.LIST_N)
    yield e
    e.close()


@pytest.fixture(scope="module")
def raw(emu_lib):
    e = ac.make_engine(emu_lib, "raw", 4)
    yield e
    e.close()


@pytest.fixture(scope="module", params=("am", "am-pipe"))
def am(emu_lib, request):
    e = ac.make_engine(emu_lib, request.param)
    yield e
    e.close()


@pytest.mark.parametrize("name", aa.single_names("fm"))
def test_fm_acquisition_equals_the_twins_on_the_emulated_build(fifo, oracle, name):
    ac.check_single(fifo, oracle, "fm", name)


def test_fm_acquisition_leaves_fine_and_short_streams_alone_on_the_emulated_build(fifo):
    ac.check_inactive(fifo, "fm")


def test_fm_acquisition_walks_a_list_of_65_active_streams_on_the_emulated_build(fifo, oracle):
    active, n = ac.check_list(fifo, oracle, LIST_N_EMU)
    assert active >= 65 and n == 95


def test_fm_acquisition_decimates_its_window_at_rd_on_the_emulated_build(raw, oracle):
    ac.check_raw(raw, oracle)


@pytest.mark.parametrize("name", aa.single_names("am"))
def test_am_acquisition_equals_the_twins_on_the_emulated_build(am, oracle, name):
    ac.check_single(am, oracle, "am", name)


def test_am_acquisition_leaves_fine_and_short_streams_alone_on_the_emulated_build(am):
    ac.check_inactive(am, "am")


def test_fifo_hook_rejects_bad_arguments(fifo):
    ac.check_rejections_fifo(fifo)


def test_zero_copy_hook_rejects_bad_arguments(raw):
    ac.check_rejections_raw(raw)


def test_am_hook_rejects_bad_arguments(am):
    ac.check_rejections_am(am)


# ---- the sets --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", aa.single_names("fm"))
def test_fm_sets_hold_what_they_are_named_for(oracle, name):
    ac.check_set(oracle, "fm", name)


@pytest.mark.parametrize("name", aa.single_names("am"))
def test_am_sets_hold_what_they_are_named_for(oracle, name):
    ac.check_set(oracle, "am", name)


def test_list_set_has_65_active_streams_in_the_fixed_pattern(oracle):
    aa.use(oracle)
    assert aa.LIST_N == 95 and ac.check_set_list(aa.LIST_N) == 65 and ac.check_set_list(LIST_N_EMU) >= 33


def test_raw_set_reads_three_distinct_windows_of_uniform_bytes(oracle):
    ac.check_set_raw(oracle)
