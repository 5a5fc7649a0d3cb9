"""`-m "not gpu"`: the FM symbol transform (k_mixfft in every form, k_mixfft8) on the CPU-emulated twin through nrsc5hip_stage_symbols, against the float64 model of
tests/sym_model.py on the inputs of tests/sym_args.py (tests/sym_checks.py says what is compared); tests/test_gpu_symbol_stage.py runs the same checks on the gfx950
code.  Also here, with no device involved: the three tests of the inputs themselves -- the reference's float32 arithmetic stays within SYM_ERR_MEASURED, no bound
exceeds 1e-4 of its symbol's largest bin, every tone's expected slot is the model's arg-max."""
import pytest

from tests import sym_args as sa, sym_checks as sc


@pytest.fixture(scope="module")
def E(emu_lib):
    e = sc.make_engine(emu_lib)
    yield e
    e.close()


@pytest.mark.parametrize("form", sa.FORMS)
@pytest.mark.parametrize("name", sc.CALLS)
def test_symbols_equal_the_model_on_the_emulated_build(E, name, form):
    sc.check_call(E, name, form)


@pytest.mark.parametrize("name", sc.CALLS)
def test_symbol_forms_leave_the_same_bits_on_the_emulated_build(E, name):
    sc.check_forms(E, name)


@pytest.mark.parametrize("form", (1, 32))
def test_symbols_from_a_capture_equal_symbols_from_the_fifo_on_the_emulated_build(E, form):
    sc.check_raw_equals_fifo(E, form)


@pytest.mark.parametrize("form", sa.FORMS)
def test_symbols_fused_and_separate_prepare_agree_on_the_emulated_build(E, form):
    sc.check_prepare(E, form)


def test_symbol_hook_rejects_bad_arguments(E):
    sc.check_rejections(E)


# ---- the inputs themselves -------------------------------------------------------------------------------------------------------------------------------
def test_reference_arithmetic_stays_within_the_measured_error(oracle):
    sc.check_reference_arithmetic(oracle)


def test_no_bound_exceeds_1e_4_of_the_largest_bin():
    sc.check_bounds_are_tight()


def test_every_tone_lands_in_its_slot_in_the_model():
    sc.check_tone_cases()
