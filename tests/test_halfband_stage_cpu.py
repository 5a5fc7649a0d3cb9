"""`-m "not gpu"`: nrsc5hip_stage_halfband_raw on the CPU-emulated twin -- the production load / unpack / pairing code of all three forms
of the fused half-band (csrc/halfband_raw.h, mixfft_body.h, k_mixfft.hip) against the integer code on every set and request of
tests/halfband_args.py: which dword feeds which product, the stream-start branch, the last work-item's clamped loads, the 4 / 5 split of
the 256-lane form, the placement of the capture.  What the twin cannot show -- the inline assembly's operand lists, the byte-conversion
instructions, the rounding-mode switch -- is the device test's: tests/test_gpu_halfband_stage.py runs the same checks on the gfx950 code.
Also here: the argument checks of the hook, and that the sets hold what they are meant to hold."""
import numpy as np
import pytest

from tests import halfband_args as ha, halfband_checks as hc


@pytest.fixture(scope="module")
def E(emu_lib):
    e = hc.make_engine(emu_lib)
    yield e
    e.close()


@pytest.mark.parametrize("name", ha.SET_NAMES)
def test_halfband_forms_equal_the_integer_code_on_the_emulated_build(E, oracle, name):
    compared = hc.check_set(E, oracle, name)
    want = len(ha.LEADS) * sum(n for _, n in ha.requests(name)) * ha.SYM_N
    assert all(c == want for c in compared.values()), compared


def test_acquisition_form_across_workgroups_on_the_emulated_build(E, oracle):
    hc.check_acq_span(E, oracle)


def test_stage_halfband_raw_rejects_bad_arguments(E):
    hc.check_rejections(E)


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
def test_sets_reach_every_byte_lane_value_and_both_ends_of_every_pair_sum():
    """every byte value in each of the four byte lanes of a dword (I and Q of the even raw sample: the products; of the odd one: the
    centre), in the random set and in the slipping ramp each on its own (the plain ramps (k i) mod 256 show a lane the 64 values of its
    residue modulo 4, the four lanes together all 256); the sum of the two bytes a tap multiplies at 0 and at 510 -- s = -254 and
    +256 in the kernels' terms, the two ends of its range -- on each of the four taps, in both components"""
    for name in ("uniform", "ramp_slip"):
        lanes = ha.get(name).reshape(-1, 4)
        for lane in range(4):
            assert np.unique(lanes[:, lane]).size == 256, (name, lane)
    for name in ("ramp1", "ramp3", "ramp37"):
        lanes = ha.get(name).reshape(-1, 4)
        assert all(np.unique(lanes[:, lane]).size == 64 for lane in range(4)) and np.unique(lanes).size == 256, name
    lo = np.full((4, 2), 1 << 20)
    hi = np.zeros((4, 2), dtype=np.int64)
    for name in ha.SET_NAMES:
        s = ha.pair_byte_sums(ha.get(name))
        lo, hi = np.minimum(lo, s.min(axis=0)), np.maximum(hi, s.max(axis=0))
    assert (lo == 0).all() and (hi == 510).all(), (lo, hi)
    assert (ha.pair_byte_sums(ha.get("even0_odd255")) == 0).all() and (ha.pair_byte_sums(ha.get("even255_odd0")) == 510).all()   # every product of every output
    s = ha.pair_byte_sums(ha.get("fullscale"))
    assert (s.min(axis=0) == 0).all() and (s.max(axis=0) == 510).all()
    near = ha.pair_byte_sums(ha.get("near127")) - 254                        # products next to zero, of both signs and zero itself
    assert set(np.unique(near).tolist()) == {-2, -1, 0, 1, 2}
    assert {int(v) for v in np.unique(ha.get("near127"))} == {126, 127, 128}


def test_sets_tell_the_rounding_modes_apart(oracle):
    """A condition on the INPUTS, not on the kernels: were a device form to round its four products otherwise than downwards, the
    random-uniform set must show it.  The chain acc <- acc + R(s t_i / 512) with R = round-to-nearest-even (the mode the kernel is entered
    in: what an ineffective mode switch would compute) and with R = truncation toward zero (what a float -> int conversion in place of
    floorf would compute) differs from the integer code on 99.59 % and 99.61 % of the set's 142 571 outputs (measured; at least one of the
    eight products of an output is affected almost always); 1 % is asserted.
    (A hardware round-toward-ZERO mode could not be told from round-down by the symbol forms, and would be as correct: their accumulator
    carries HB_BIAS and is positive throughout.)"""
    iq = ha.get("uniform")
    exp = hc.reference(oracle, "uniform").astype(np.int64)
    assert np.array_equal(ha.model(iq, "floor"), exp)                       # the model itself, with the floor, is the integer code
    shares = {}
    for rounding in ("nearest", "trunc"):
        shares[rounding] = float((ha.model(iq, rounding) != exp).any(axis=1).mean())
        assert shares[rounding] >= 0.01, shares
    print("share of outputs a wrong rounding changes:", shares)
