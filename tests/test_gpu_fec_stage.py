"""GPU: the FEC stage's permutations, error counts and descramblers as the gfx950 code computes them, through the nrsc5hip_stage_* hooks that
run the production kernels on caller data -- k_p1_deint, the PIDS gather and k_pids_decode, k_px_deint + k_px_commit, k_am_interleave with its
delay ring, k_p1_forward / _fix / the traceback in both forms with the re-encode count and the descramble, am_bit_errors + am_descramble --
against the oracle's twins on the inputs of tests/fec_args.py.  Every output equal, no tolerance (tests/fec_checks.py); the same checks run on
the emulated build in tests/test_fec_stage_cpu.py, which also holds the tests of the input sets themselves."""
import pytest

from tests import fec_args as fa, fec_checks as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E(hip_lib):
    e = fc.make_engine(hip_lib)
    yield e
    e.close()


@pytest.mark.parametrize("which", ("planes", "random"))
def test_gpu_p1_deinterleave_equals_the_twin(E, oracle, which):
    assert fc.check_p1_deint(E, oracle, which) == (3 if which == "planes" else 1) * 438528


@pytest.mark.parametrize("which", ("planes", "random", "encoded"))
def test_gpu_pids_gather_decode_and_crc_equal_the_twins(E, oracle, which):
    flags = [fc.check_pids(E, oracle, which, bc) for bc in range(16)]
    if which == "encoded":
        assert sum(f[0] for f in flags) == 14


@pytest.mark.parametrize("length", fa.PX_LENS)
@pytest.mark.parametrize("which", ("planes", "random"))
def test_gpu_interleaver_iv_equals_the_twin_over_36_pairs(E, oracle, which, length):
    assert fc.check_px(E, oracle, which, length) == (3 if which == "planes" else 1) * fa.PX_PAIRS * 2 * 3 * length


@pytest.mark.parametrize("psmi", (fa.MA1, fa.MA3))
@pytest.mark.parametrize("which", ("planes", "random"))
def test_gpu_am_deinterleave_and_delay_ring_equal_the_twin(E, oracle, which, psmi):
    fc.check_am(E, oracle, which, psmi)


@pytest.mark.parametrize("segments", (1, 4))
@pytest.mark.parametrize("walk", (0, 1))
@pytest.mark.parametrize("name", fa.P1_FRAMES)
def test_gpu_p1_error_count_and_descramble_equal_the_twins(E, oracle, name, walk, segments):
    fc.check_p1_frame(E, oracle, name, walk, segments)


@pytest.mark.parametrize("threads", (64, 256))
@pytest.mark.parametrize("kind", ("random", "codeword"))
@pytest.mark.parametrize("length,code", fa.AM_FRAMES)
def test_gpu_am_error_count_and_descramble_equal_the_twins(E, oracle, length, code, kind, threads):
    fc.check_am_epilogue(E, oracle, length, code, kind, threads)


def test_gpu_fec_stage_hooks_reject_bad_arguments(E):
    fc.check_rejections(E)
