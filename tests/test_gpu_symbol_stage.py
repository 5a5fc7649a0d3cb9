"""GPU: the FM symbol transform as the gfx950 code computes it -- k_mixfft<1 / 2 / 4 / 8, 1>, k_mixfft<1, 2> and k_mixfft8, launched alone by
nrsc5hip_stage_symbols -- against the float64 model of tests/sym_model.py on the inputs of tests/sym_args.py: every live bin of every symbol within the bound derived
there, nothing else written, the 128-lane forms bit-identical, capture and FIFO bit-identical, fused and separate bookkeeping bit-identical, every tone in its slot
(tests/sym_checks.py).  The same checks run on the emulated build in tests/test_symbol_stage_cpu.py, which also tests the inputs themselves.  One block per hook
call, one engine for the module."""
import pytest

from tests import sym_args as sa, sym_checks as sc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


@pytest.fixture(scope="module")
def E(hip_lib):
    e = sc.make_engine(hip_lib)
    yield e
    e.close()


@pytest.mark.parametrize("form", sa.FORMS)
@pytest.mark.parametrize("name", sc.CALLS)
def test_gpu_symbols_equal_the_model(E, name, form):
    sc.check_call(E, name, form)


@pytest.mark.parametrize("name", sc.CALLS)
def test_gpu_symbol_forms_leave_the_same_bits(E, name):
    sc.check_forms(E, name)


@pytest.mark.parametrize("form", (1, 32))
def test_gpu_symbols_from_a_capture_equal_symbols_from_the_fifo(E, form):
    sc.check_raw_equals_fifo(E, form)


@pytest.mark.parametrize("form", sa.FORMS)
def test_gpu_symbols_fused_and_separate_prepare_agree(E, form):
    sc.check_prepare(E, form)


def test_gpu_symbol_hook_rejects_bad_arguments(E):
    sc.check_rejections(E)
