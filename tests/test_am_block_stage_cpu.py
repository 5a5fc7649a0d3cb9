"""`-m "not gpu"`: the AM block step (k_am_block) on the CPU-emulated twin through nrsc5hip_stage_am_block, in both launch forms, against the float64 model of
tests/am_model.py on the input sets of tests/am_args.py (tests/am_checks.py says what is compared); tests/test_gpu_am_block_stage.py runs the same checks on the gfx950
code.  Also here, with no device involved: the model pinned to the oracle's log of two golden captures -- which is where the spectrum bound is measured -- and what
the input sets hold."""
import numpy as np
import pytest

from oracle import port
from tests import am_args as aa, am_checks as ac, am_model as M, common

CASES = [(w, n) for w in ("refseq", "cells", "edge", "carrier", "inactive") for n in aa.names(w)]


@pytest.fixture(scope="module")
def engines(emu_lib):
    es = {k: ac.make_engine(emu_lib, k) for k in ("am", "am-pipe")}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("form", ("am", "am-pipe"))
@pytest.mark.parametrize("which,name", CASES)
def test_am_block_equals_the_model_on_the_emulated_build(engines, oracle, form, which, name):
    ac.check_case(engines[form], oracle, which, name)


@pytest.mark.parametrize("which", list(aa.SETS))
def test_am_block_256_and_512_lanes_leave_the_same_bytes_on_the_emulated_build(engines, which):
    ac.check_shapes(engines["am"], engines["am-pipe"], which)


@pytest.mark.parametrize("form", ("am", "am-pipe"))
@pytest.mark.parametrize("which", list(aa.SETS))
def test_am_block_dump_changes_no_output_on_the_emulated_build(engines, form, which):
    ac.check_dump(engines[form], which)


@pytest.mark.parametrize("form", ("am", "am-pipe"))
def test_am_block_hook_rejects_bad_arguments(engines, form):
    ac.check_rejections(engines[form])


def test_am_block_hook_needs_an_am_engine(emu_lib):
    ac.check_rejects_engine_without_am(emu_lib)


# ---- the model, pinned to the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("am_cs16_cfo3", "am_ma3_cs16"))
def test_model_reproduces_the_oracle_log(oracle, captures, name):
    """The model as a receiver over the oracle's Q15 stream: the integer block trace exactly, every hard symbol whose model distance exceeds its margin, the record
    floats within tests/common.py's bounds, the sync event, and the oracle's float32 spectra within SPEC_ERR_MEASURED of the block's largest bin"""
    log, q15, fft = oracle.run(captures(name).iq, taps=port.TAP_Q15 | port.TAP_FFT | port.TAP_SOFT, fft_blocks=1 << 20, mode=1)
    blocks = [v for k, v in log if k == "block"]
    syms = iter([v for k, v in log if k == "amsym"])
    syncs = iter([v for k, v in log if k == "sync"])
    outs = M.receive(q15)
    fft = fft.reshape(-1, M.NSYM, M.FFT)
    assert len(outs) == len(blocks) == len(fft) and any(o["rec"]["state_after"] == M.FINE for o in outs)
    idx = np.arange(-81, 82) % M.FFT
    worst, cells, out_cells = 0.0, 0, 0
    for b, (o, r) in enumerate(zip(outs, blocks)):
        for k in ("state_before", "state_after", "samperr", "cfo", "keep", "bc", "psmi", "cfo_wait", "next_samperr"):
            assert o["rec"][k] == r[k], "block %d: %s is %d, the oracle's %d" % (b, k, o["rec"][k], r[k])
        for k in ("prev_angle", "phase_re", "phase_im", "next_angle"):
            assert common.float_close(k, r[k], o["rec"][k]), "block %d: %s is %r, the oracle's %r" % (b, k, o["rec"][k], r[k])
        ref = np.fft.ifftshift(fft[b].astype(np.complex128), axes=1)
        worst = max(worst, float(np.abs(ref - o["spectra_raw"])[:, idx].max() / np.abs(ref).max()))
        if o["rec"]["flags"] & M.REC_TO_FINE:
            ev = next(syncs)
            assert common.float_close("freq_offset", ev["freq_offset"], o["rec"]["freq_offset"]), (b, ev, o["rec"]["freq_offset"])
            assert (ev["psmi"], ev["pli"], ev["hppi"], ev["aabi"], ev["rdbi"]) == tuple(o["state"][k] for k in ("psmi", "pli", "hppi", "aabi", "rdbi"))
        if "sym" in o:
            s = next(syms)
            assert s["bc"] == o["rec"]["bc_decoded"], (b, s["bc"], o["rec"]["bc_decoded"])
            bad = np.stack([s["pl"], s["pu"], s["s"], s["t"]]) != o["sym"]
            out_cell, _ = aa.excluded(o, aa.margins(o))
            cells += bad.size; out_cells += int(out_cell.sum())
            assert not (bad & ~out_cell).any(), "block %d: %d cells differ from the oracle's, the first %.4g grid units from a boundary" % (b, bad.sum(), o["dist"][bad][0])
    assert next(syms, None) is None and next(syncs, None) is None
    print("%s: oracle float32 spectra vs float64 model: %.3g of the largest bin (bound %.3g); %d of %d cells within their margin" % (name, worst, aa.SPEC_ERR_MEASURED, out_cells, cells))
    assert worst <= aa.SPEC_ERR_MEASURED, worst
    assert out_cells <= 0.01 * cells


# ---- the sets, on the model alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,name", CASES)
def test_am_sets_hold_what_they_are_named_for(which, name):
    ac.check_set(which, name)


def test_cells_set_sends_every_point_on_every_carrier():
    ac.check_cover()
