"""GPU: csrc/fastmath.h as the gfx950 code evaluates it (nrsc5hip_stage_math), on the argument sets of tests/math_args.py under the
checks of tests/math_checks.py.  ref_sincosf / ref_atan2f against this host's libm, bit for bit, on every argument: the float divisions
(denormal quotients and operands included), the 64-bit reduction of large arguments with its table path -- which no Costas loop reaches,
so no end-to-end test vouches for it -- and the absence of contraction are properties of the device build only.  The double series
against the g++ build of the same header, bit for bit, and against extended precision.  The fast forms (v_sin_f32 / v_cos_f32 /
v_rcp_f32) against float64: the header's own figures, SURVEY 8c's 1e-4, and the exact properties."""
import pytest

from nrsc5_amd import engine as eng
from tests import math_args as ma, math_checks as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E(hip_lib):
    e = mc.make_engine(hip_lib)
    yield e
    e.close()


def test_gpu_ref_sincosf_equals_host_libm_bit_for_bit(E):
    if not mc.host_has_fma():
        pytest.skip("host CPU without FMA + AVX2: its glibc dispatches to the unfused sincosf")
    assert mc.check_ref_sincosf(E, ma.get("sincosf")) == ma.N_DEVICE


def test_gpu_ref_atan2f_equals_host_libm_bit_for_bit(E):
    assert mc.check_ref_atan2f(E, ma.get("atan2f")) == ma.N_DEVICE_ATAN2F


def test_gpu_series_equal_the_host_build_and_stay_within_two_ulps(E, emu_lib):
    cs, at = ma.get("small_cos_sin"), ma.get("small_atan")
    dev = mc.series_results(E, cs, at)
    host = mc.make_engine(emu_lib)
    try:
        mc.check_series_equal(dev, mc.series_results(host, cs, at))
    finally:
        host.close()
    mc.check_series(dev, cs, at)


def test_gpu_fast_sincos_within_the_header_figure(E):
    mc.check_fast_sincos(E, ma.get("fast_sincos"))


def test_gpu_fast_sincos_reduced_within_the_header_figure(E):
    mc.check_fast_sincos(E, ma.get("fast_sincos_reduced"), fn=eng.MATH_FAST_SINCOS_REDUCED)


def test_gpu_fast_atan2_within_the_header_figure(E):
    mc.check_fast_atan2(E, ma.get("fast_atan2"))
