"""`-m "not gpu"`: the FEC stage hooks on the CPU-emulated twin -- the production kernels' indexing, their tables (engine.hip: build_tables) and
their bookkeeping against the oracle's twins, bit for bit, on the inputs of tests/fec_args.py (tests/fec_checks.py says what is compared and
why the end-to-end tests cannot see it).  What only the device can show -- the generated code of the same kernels -- is
tests/test_gpu_fec_stage.py's, which runs the same checks.  Also here: the argument checks of the hooks, and what the input sets hold."""
import numpy as np
import pytest

from tests import fec_args as fa, fec_checks as fc


@pytest.fixture(scope="module")
def E(emu_lib):
    e = fc.make_engine(emu_lib)
    yield e
    e.close()


@pytest.mark.parametrize("which", ("planes", "random"))
def test_p1_deinterleave_equals_the_twin_on_the_emulated_build(E, oracle, which):
    assert fc.check_p1_deint(E, oracle, which) == (3 if which == "planes" else 1) * 438528


@pytest.mark.parametrize("which", ("planes", "random", "encoded"))
def test_pids_gather_decode_and_crc_equal_the_twins_on_the_emulated_build(E, oracle, which):
    flags = [fc.check_pids(E, oracle, which, bc) for bc in range(16)]
    if which == "encoded":
        assert sum(f[0] for f in flags) == 14                                  # both values of the CRC flag are seen


@pytest.mark.parametrize("length", fa.PX_LENS)
@pytest.mark.parametrize("which", ("planes", "random"))
def test_interleaver_iv_equals_the_twin_over_36_pairs_on_the_emulated_build(E, oracle, which, length):
    assert fc.check_px(E, oracle, which, length) == (3 if which == "planes" else 1) * fa.PX_PAIRS * 2 * 3 * length


@pytest.mark.parametrize("psmi", (fa.MA1, fa.MA3))
@pytest.mark.parametrize("which", ("planes", "random"))
def test_am_deinterleave_and_delay_ring_equal_the_twin_on_the_emulated_build(E, oracle, which, psmi):
    fc.check_am(E, oracle, which, psmi)


@pytest.mark.parametrize("segments", (1, 4))
@pytest.mark.parametrize("walk", (0, 1))
@pytest.mark.parametrize("name", fa.P1_FRAMES)
def test_p1_error_count_and_descramble_equal_the_twins_on_the_emulated_build(E, oracle, name, walk, segments):
    fc.check_p1_frame(E, oracle, name, walk, segments)


@pytest.mark.parametrize("threads", (64, 256))
@pytest.mark.parametrize("kind", ("random", "codeword"))
@pytest.mark.parametrize("length,code", fa.AM_FRAMES)
def test_am_error_count_and_descramble_equal_the_twins_on_the_emulated_build(E, oracle, length, code, kind, threads):
    fc.check_am_epilogue(E, oracle, length, code, kind, threads)


def test_fec_stage_hooks_reject_bad_arguments(E):
    fc.check_rejections(E)


def test_am_deinterleave_hook_needs_an_am_engine(emu_lib):
    fc.check_am_hook_needs_am_engine(emu_lib)


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
def test_matrix_planes_name_every_cell_and_the_interleavers_tile_the_matrices(oracle):
    fc.check_sets_pm(oracle)


@pytest.mark.parametrize("length", fa.PX_LENS)
def test_pair_planes_name_every_cell_and_interleaver_iv_reads_each_once(oracle, length):
    fc.check_sets_px(oracle, length)


@pytest.mark.parametrize("psmi", (fa.MA1, fa.MA3))
def test_am_planes_name_every_bit_and_interleaver_ma1_reads_each_once(oracle, psmi):
    fc.check_sets_am(oracle, psmi)


def test_frames_reach_the_edges_they_are_named_for(oracle):
    """conditions on the INPUTS: the noise frame and the random matrices hold every byte value, -128 among them; the code-word frame decodes
    (by the twin) to its code word although it holds zeros, -128 and wrong signs at both sides of the wrap and of chunk boundaries; its
    punctured wrong signs are not counted; the AM code-word frames put a wrong sign on a punctured place (E2, phase 5) and on unpunctured ones"""
    for x in (fa.p1_frame("noise"), fa.pm_random(), fa.px_random(2304), fa.px_random(4608)):
        assert np.unique(x).size == 256
    assert np.unique(fa.am_random()).size == 256
    soft = fa.p1_frame("codeword").reshape(-1, 3)
    info, cw = fa.p1_codeword()
    wrong = (soft > 0) != (cw == 1)
    steps = np.flatnonzero(wrong.any(axis=1))
    assert set(range(6)) <= set(steps) and set(range(fa.P1_LEN - 6, fa.P1_LEN)) <= set(steps)
    for edge in (64, 128, 64000, fa.P1_LEN - 64):
        assert edge - 1 in steps and edge in steps
    assert wrong[1000, 2] and wrong[1001, 2] and (soft == 0).sum() == len(fa.K7_ZEROS) and (soft == -128).sum() == 8
    unpunct = np.ones_like(wrong); unpunct[1::2, 2] = False
    assert (wrong & unpunct).sum() == fa.p1_codeword_expected() == 25 and (wrong & ~unpunct).sum() == 3
    assert np.array_equal(fc.ref_p1_frame(oracle, "codeword")[0], info)
    assert fc.ref_p1_frame(oracle, "codeword")[2] == 25
    # full-range noise: about 0.2 x 365440 disagreements (the decoder fits a code word to the noise)
    assert 0.15 * fa.P1_CODED < fc.ref_p1_frame(oracle, "noise")[2] < 0.3 * fa.P1_CODED
    for length, code in fa.AM_FRAMES:
        plen = len(fa.AM_PUNCT[code])
        places = np.array(fa.am_flip_places(length, code))
        assert {0, plen - 1} <= set((places[(places >= 24) & (places < 3 * length - 24)] % plen).tolist())
        assert places.min() == 0 and places.max() == 3 * length - 1
        assert fa.am_frame(length, code, "codeword")[2] == int(np.resize(fa.AM_PUNCT[code], 3 * length)[places].sum()) < places.size
