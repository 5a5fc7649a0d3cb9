"""`-m "not gpu"`: nrsc5hip_stage_math on the CPU-emulated twin -- the hook itself (every function, the argument checks) and the
checks of tests/math_checks.py on the 2^16 subsets of tests/math_args.py: ref_sincosf / ref_atan2f bit-equal to this host's libm, the
double series within 2 ulps.  The same checks run on the gfx950 code in tests/test_gpu_math_stage.py; the fast forms are checked there
only (here they are libm).  Also here: the argument sets hold what they are meant to hold."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import math_args as ma, math_checks as mc


@pytest.fixture(scope="module")
def E(emu_lib):
    e = mc.make_engine(emu_lib)
    yield e
    e.close()


def test_ref_sincosf_on_the_emulated_build(E):
    if not mc.host_has_fma():
        pytest.skip("host CPU without FMA + AVX2: its glibc dispatches to the unfused sincosf")
    assert mc.check_ref_sincosf(E, ma.get("sincosf", emu=True)) >= 60000


def test_ref_atan2f_on_the_emulated_build(E):
    assert mc.check_ref_atan2f(E, ma.get("atan2f", emu=True)) >= 60000


def test_series_within_two_ulps_on_the_emulated_build(E):
    cs, at = ma.get("small_cos_sin", emu=True), ma.get("small_atan", emu=True)
    mc.check_series(mc.series_results(E, cs, at), cs, at)


def test_fast_forms_run_on_the_emulated_build(E):
    """libm behind the fast forms' names: the hook's plumbing (two inputs, two outputs, float) and nothing about accuracy"""
    x = ma.get("fast_sincos", emu=True)
    for fn in (eng.MATH_FAST_SINCOS, eng.MATH_FAST_SINCOS_REDUCED):
        s, c = E.stage_math(fn, x.a)
        assert np.abs(s.astype(np.float64) - np.sin(x.a.astype(np.float64))).max() < 1e-6 and np.abs(c.astype(np.float64) - np.cos(x.a.astype(np.float64))).max() < 1e-6
    a = ma.get("fast_atan2", emu=True)
    r = E.stage_math(eng.MATH_FAST_ATAN2, a.a, a.b)
    assert np.abs(r.astype(np.float64) - np.arctan2(a.a.astype(np.float64), a.b.astype(np.float64))).max() < 1e-6


def test_stage_math_rejects_bad_arguments(E):
    one = np.ones(4, dtype=np.float32)
    with pytest.raises(eng.Nrsc5HipError) as ei:
        E._check(E.lib.nrsc5hip_stage_math(E._h, 7, one.ctypes.data, None, 4, one.ctypes.data, one.ctypes.data))
    assert ("error %d:" % eng.EINVAL) in str(ei.value)
    for fn, b, out1 in ((eng.MATH_REF_ATAN2F, None, None), (eng.MATH_REF_SINCOSF, None, None), (eng.MATH_SMALL_ATAN, None, None)):
        out = np.zeros(4, dtype=np.float64)
        n = 0 if fn == eng.MATH_SMALL_ATAN else 4             # the series with nothing to do; the others with a missing array
        with pytest.raises(eng.Nrsc5HipError) as ei:
            E._check(E.lib.nrsc5hip_stage_math(E._h, fn, out.ctypes.data, b, n, out.ctypes.data, out1))
        assert ("error %d:" % eng.EINVAL) in str(ei.value)
    with pytest.raises(ValueError):
        E.stage_math(eng.MATH_REF_ATAN2F, one)
    with pytest.raises(ValueError):
        E.stage_math(eng.MATH_REF_SINCOSF, one, one)


def test_one_element_and_a_partial_workgroup(E):
    """n = 1 and n = 257: one lane of one workgroup, and a second workgroup of one lane"""
    t = np.linspace(-0.26, 0.26, 257)
    full = E.stage_math(eng.MATH_SMALL_ATAN, t)
    assert np.abs(full - np.arctan(t)).max() < 1e-15
    assert E.stage_math(eng.MATH_SMALL_ATAN, t[:1])[0] == full[0]


# ---- the argument sets ---------------------------------------------------------------------------------------------------------------
def test_sincosf_set_reaches_every_path():
    s = ma.get("sincosf")
    assert len(s) == ma.N_DEVICE and len(ma.get("sincosf", emu=True)) <= ma.N_EMU
    u = ma.bits(s.a)
    top = (u >> 20) & 0x7ff
    large = (top >= 0x42f) & (top < 0x7f8)
    assert set(((u[large] >> 26) & 15).tolist()) == set(range(16)) and set(((u[large] >> 23) & 7).tolist()) == set(range(8))
    for sub in (s, ma.get("sincosf", emu=True)):
        t = (ma.bits(sub.a) >> 20) & 0x7ff
        for lo, hi in ((0, 0x398), (0x398, 0x3f4), (0x3f4, 0x42f), (0x42f, 0x7f8), (0x7f8, 0x800)):
            assert ((t >= lo) & (t < hi)).sum() >= 64, (lo, hi)
        assert (((ma.bits(sub.a) >> 26) & 15)[(t >= 0x42f) & (t < 0x7f8)] > 3).sum() >= 1000      # the table path
    for thr in ma.SINCOSF_TOPS:                                                                  # 64 floats on either side, both signs
        for sign in (0, 0x80000000):
            want = (np.arange(-64, 64, dtype=np.int64) + (thr << 20)) | sign
            assert np.isin(want.astype(np.uint32), u).all(), hex(thr)


def test_atan2f_set_reaches_every_path():
    s = ma.get("atan2f")
    assert len(s) == ma.N_DEVICE_ATAN2F and len(ma.get("atan2f", emu=True)) <= ma.N_EMU
    iy, ix = (ma.bits(s.a) & 0x7fffffff).astype(np.int64), (ma.bits(s.b) & 0x7fffffff).astype(np.int64)
    k = (iy - ix) >> 23
    finite = (iy < 0x7f800000) & (ix < 0x7f800000) & (iy > 0) & (ix > 0)
    for kk in range(57, 64):
        assert (finite & (k == kk)).sum() >= 256 and (finite & (k == -kk)).sum() >= 256, kk
    den_y, den_x = (iy > 0) & (iy < 0x800000), (ix > 0) & (ix < 0x800000)
    assert (den_y & den_x).sum() >= 4096 and (~den_y & den_x & finite).sum() >= 4096 and (den_y & ~den_x & finite).sum() >= 2048
    with np.errstate(all="ignore"):
        q = np.abs(s.a / s.b)                                                                    # float32 division on the host
    normal = finite & ~den_y & ~den_x
    assert (normal & (q > 0) & (q < np.float32(2.0 ** -126))).sum() >= 2048 and (normal & (q == 0)).sum() >= 512
    assert (ma.bits(s.b) == 0x3f800000).sum() >= 16384
    for thr in ma.ATANF_THRESHOLDS:                                                              # both sides of every ratio threshold, in every quadrant
        part = s.only("ratio %g" % thr)
        with np.errstate(all="ignore"):
            r = np.abs(part.a / part.b)
        for sy, sx in ma.QUADRANTS:
            m = (np.signbit(part.a) == (sy < 0)) & (np.signbit(part.b) == (sx < 0))
            assert (m & (r < np.float32(thr))).sum() >= 2048 * 20 and (m & (r >= np.float32(thr))).sum() >= 2048 * 20, (thr, sy, sx)
