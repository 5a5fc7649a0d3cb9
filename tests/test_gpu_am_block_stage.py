"""GPU: the AM block step as the gfx950 code computes it -- k_am_block<256> in order and k_am_block<512> as the window pipeline launches it, launched alone by
nrsc5hip_stage_am_block -- against the float64 model of tests/am_model.py on the input sets of tests/am_args.py: integers exact, hard symbols exact outside the
model's margins, floats and the dumped tile within the bounds derived there (tests/am_checks.py).  The same checks run on the emulated build in
tests/test_am_block_stage_cpu.py, which also pins the model to the oracle and tests the sets themselves.  One block per hook call, one engine per launch form."""
import pytest

from tests import am_args as aa, am_checks as ac

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
CASES = [(w, n) for w in ("refseq", "cells", "edge", "carrier", "inactive") for n in aa.names(w)]


@pytest.fixture(scope="module")
def engines(hip_lib):
    es = {k: ac.make_engine(hip_lib, k) for k in ("am", "am-pipe")}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("form", ("am", "am-pipe"))
@pytest.mark.parametrize("which,name", CASES)
def test_gpu_am_block_equals_the_model(engines, oracle, form, which, name):
    ac.check_case(engines[form], oracle, which, name)


@pytest.mark.parametrize("which", list(aa.SETS))
def test_gpu_am_block_256_and_512_lanes_leave_the_same_bytes(engines, which):
    ac.check_shapes(engines["am"], engines["am-pipe"], which)


@pytest.mark.parametrize("form", ("am", "am-pipe"))
@pytest.mark.parametrize("which", list(aa.SETS))
def test_gpu_am_block_dump_changes_no_output(engines, form, which):
    ac.check_dump(engines[form], which)


@pytest.mark.parametrize("form", ("am", "am-pipe"))
def test_gpu_am_block_hook_rejects_bad_arguments(engines, form):
    ac.check_rejections(engines[form])


def test_gpu_am_block_hook_needs_an_am_engine(hip_lib):
    ac.check_rejects_engine_without_am(hip_lib)
