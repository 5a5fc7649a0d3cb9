"""GPU: the fused float32 half-band (csrc/halfband_raw.h) as the gfx950 code evaluates it, through nrsc5hip_stage_halfband_raw: the three
forms the zero-copy batch runs -- hb_sample_q15 (k_acq_decimate), raw_symbol_load + raw_symbol_halfband (k_mixfft: v_pk_fma_f32 under
round-toward-minus-infinity), raw_symbol_load8 + raw_symbol_halfband8 (k_mixfft8: taps in scalar register pairs) -- called by stage kernels
of the production workgroup sizes, against oracle.halfband_fm_cu8 (the C restatement of firdecim_q15.c) on the sets and requests of
tests/halfband_args.py.  Every output equal, no tolerance: full-scale and near-zero input, every byte value in every byte lane, the
stream-start branch, the last work-item's clamped loads, every dword alignment of the capture.  What only the device can show is in here:
the v_cvt_f32_ubyte* unpacking, the operand lists of the inline assembly, and that s_setreg_imm32_b32 switches the rounding (the data
would differ on 99.6 % of the random outputs if it did not: tests/test_halfband_stage_cpu.py) and puts it back with the denormal bits
untouched (the probes)."""
import pytest

from tests import halfband_args as ha, halfband_checks as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E(hip_lib):
    e = hc.make_engine(hip_lib)
    yield e
    e.close()


@pytest.mark.parametrize("name", ha.SET_NAMES)
def test_gpu_halfband_forms_equal_the_integer_code(E, oracle, name):
    compared = hc.check_set(E, oracle, name)
    want = len(ha.LEADS) * sum(n for _, n in ha.requests(name)) * ha.SYM_N
    assert all(c == want for c in compared.values()), compared


def test_gpu_acquisition_form_across_workgroups(E, oracle):
    hc.check_acq_span(E, oracle)


def test_gpu_stage_halfband_raw_rejects_bad_arguments(E):
    hc.check_rejections(E)
