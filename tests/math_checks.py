"""Checks of csrc/fastmath.h through nrsc5hip_stage_math, shared by tests/test_math_stage_cpu.py (the CPU-emulated twin) and
tests/test_gpu_math_stage.py (the gfx950 library): the kernel evaluates the header's own functions on the argument sets of
tests/math_args.py, and

* ref_sincosf / ref_atan2f must equal the libm of the host the test runs on BIT FOR BIT on every argument (a NaN equals a NaN of any
  payload).  The expected values come from a C helper compiled with gcc that calls sincosf / atan2f -- not from numpy, whose float32
  sine is not glibc's, and not from any libm of the device;
* small_cos_sin / small_atan stay within 2 ulps of an extended-precision reference;
* fast_sincos / fast_sincos_reduced / fast_atan2 (device only: on the emulated build they are libm) stay within the figures the header
  of fastmath.h states, within SURVEY 8c's 1e-4 as the hard contract, and have the exact properties that need no tolerance."""
import functools
import os
import subprocess
import tempfile

import numpy as np

from nrsc5_amd import engine as eng

HELPER_SRC = r'''
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
/* helper <s|a> <in> <out> <n>: s = n floats y -> n sines, then n cosines; a = n floats y, then n floats x -> n angles */
int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const long n = atol(argv[4]);
    const int two = argv[1][0] == 'a';
    float *in = malloc(sizeof(float) * 2 * n), *out = malloc(sizeof(float) * 2 * n);
    FILE *f = fopen(argv[2], "rb");
    if (!in || !out || !f || fread(in, sizeof(float), (two ? 2 : 1) * n, f) != (size_t)((two ? 2 : 1) * n)) return 3;
    fclose(f);
    if (two) for (long i = 0; i < n; i++) out[i] = atan2f(in[i], in[n + i]);
    else for (long i = 0; i < n; i++) sincosf(in[i], &out[i], &out[n + i]);
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out, sizeof(float), (two ? 1 : 2) * n, f) != (size_t)((two ? 1 : 2) * n)) return 4;
    fclose(f);
    return 0;
}
'''

SIN_COS_HEADER = 5e-7           # fastmath.h: |error| of fast_sincos for |x| <= 2000 rad, and of the reduced form
ATAN2_HEADER = 3e-7             # fastmath.h: |error| of fast_atan2, rad
SURVEY_8C = 1e-4                # the hard contract for all three
SERIES_ULPS = 2.0


def host_has_fma() -> bool:
    try:
        flags = next(l for l in open("/proc/cpuinfo") if l.startswith("flags")).split()
    except (OSError, StopIteration):
        return False
    return "fma" in flags and "avx2" in flags


def _libm(mode, arrays):
    """runs the helper once: the host libm's sincosf / atan2f on float32 arrays"""
    n = arrays[0].size
    with tempfile.TemporaryDirectory() as d:
        src, exe, fin, fout = (os.path.join(d, f) for f in ("h.c", "h", "in.f32", "out.f32"))
        open(src, "w").write(HELPER_SRC)
        subprocess.check_call(["gcc", "-O2", "-fno-builtin", "-o", exe, src, "-lm"])
        np.concatenate([np.ascontiguousarray(a, dtype=np.float32) for a in arrays]).tofile(fin)
        subprocess.check_call([exe, mode, fin, fout, str(n)])
        out = np.fromfile(fout, dtype=np.float32)
    return out


@functools.lru_cache(maxsize=None)
def _libm_cached(mode, args):
    out = _libm(mode, [args.a] if args.b is None else [args.a, args.b])
    out.setflags(write=False)
    return out


def libm_sincosf(args):
    """-> (sin, cos) of args.a by the host's libm; computed once per argument set and session"""
    out = _libm_cached("s", args)
    return out[:len(args)], out[len(args):]


def libm_atan2f(args):
    return _libm_cached("a", args)


def make_engine(lib):
    return eng.Engine(max_streams=1, q15_capacity=2 * 71280, lib_path=lib)


def _hex(v):
    return "0x%08x" % int(np.asarray(v, dtype=np.float32).reshape(1).view(np.uint32)[0])


def mismatches(got, exp):
    g, e = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(exp, dtype=np.float32)
    return np.flatnonzero((g.view(np.uint32) != e.view(np.uint32)) & ~(np.isnan(g) & np.isnan(e)))


def _report(args, bad, columns):
    """the first eight failing arguments as bit patterns, with what the kernel returned and what libm returns"""
    lines = []
    for i in bad[:8]:
        arg = "y " + _hex(args.a[i]) + ("" if args.b is None else " x " + _hex(args.b[i]))
        res = "  ".join("%s got %s libm %s" % (name, _hex(g[i]), _hex(e[i])) for name, g, e in columns)
        lines.append("%s: %s  [%s]" % (arg, res, args.part_name(i)))
    return "\n".join(lines)


def check_ref_sincosf(E, args):
    """every sine and every cosine of the set bit-equal to the host libm's sincosf; -> number of arguments checked"""
    s, c = E.stage_math(eng.MATH_REF_SINCOSF, args.a)
    es, ec = libm_sincosf(args)
    bad = np.union1d(mismatches(s, es), mismatches(c, ec))
    if bad.size:
        print(_report(args, bad, (("sin", s, es), ("cos", c, ec))))
    assert bad.size == 0, "%d of %d arguments differ from the host libm's sincosf" % (bad.size, len(args))
    return len(args)


def check_ref_atan2f(E, args):
    r = E.stage_math(eng.MATH_REF_ATAN2F, args.a, args.b)
    e = libm_atan2f(args)
    bad = mismatches(r, e)
    if bad.size:
        print(_report(args, bad, (("atan2", r, e),)))
    assert bad.size == 0, "%d of %d arguments differ from the host libm's atan2f" % (bad.size, len(args))
    return len(args)


# ---- the double series -----------------------------------------------------------------------------------------------------------
def _extended(fn, x):
    """fn of float64 x in extended precision -> (values as float64-exact-or-better longdouble)"""
    if np.finfo(np.longdouble).nmant >= 63:                  # x87 extended: 11 bits beyond a double, 5e-4 ulp of a double
        return fn(x.astype(np.longdouble))
    import mpmath                                            # a platform whose long double is a double: slow, but a reference
    mpmath.mp.prec = 100
    f = {np.cos: mpmath.cos, np.sin: mpmath.sin, np.arctan: mpmath.atan}[fn]
    return np.array([float(f(mpmath.mpf(float(v)))) for v in x], dtype=np.longdouble)


def ulp_error(got, ref):
    """|got - ref| in units of the last place of a double of ref's binade; ref == 0 must be hit exactly"""
    ref = np.asarray(ref, dtype=np.longdouble)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref)
    zero = ref == 0
    _, ex = np.frexp(np.where(zero, 1.0, np.abs(ref)).astype(np.float64))           # |ref| = m 2^ex, m in [0.5, 1)
    ulp = np.ldexp(np.longdouble(1.0), (ex - 53).astype(np.int32))
    return np.where(zero, np.where(err == 0, 0.0, np.inf), err / ulp).astype(np.float64)


def series_results(E, cs_args, at_args):
    c, s = E.stage_math(eng.MATH_SMALL_COS_SIN, cs_args.a)
    return c, s, E.stage_math(eng.MATH_SMALL_ATAN, at_args.a)


def check_series(results, cs_args, at_args):
    """-> the largest error of cos, sin, atan in ulps, each asserted <= 2"""
    c, s, t = results
    worst = {}
    for name, got, fn, args in (("cos", c, np.cos, cs_args), ("sin", s, np.sin, cs_args), ("atan", t, np.arctan, at_args)):
        u = ulp_error(got, _extended(fn, args.a))
        k = int(np.argmax(u))
        worst[name] = float(u[k])
        print("small_%s: max error %.3f ulp at x = %r" % (name, u[k], float(args.a[k])))
        assert u[k] <= SERIES_ULPS, "small_%s: %.3f ulp at x = %r (%s)" % (name, u[k], float(args.a[k]), float(args.a[k]).hex())
    return worst


def check_series_equal(dev, emu):
    """IEEE double, no contraction: the device's series and the g++ build's must not differ in one bit"""
    for name, a, b in zip(("cos", "sin", "atan"), dev, emu):
        bad = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))
        assert bad.size == 0, "small_%s: %d results differ from the host build, first at index %d: %s vs %s" % (name, bad.size, bad[0], float(a[bad[0]]).hex(), float(b[bad[0]]).hex())


# ---- the fast forms (device only) ------------------------------------------------------------------------------------------------
def check_fast_sincos(E, args, fn=None, bound=SIN_COS_HEADER):
    """-> {part name: (max |error| of sin, of cos)} against float64 numpy of the same float arguments"""
    s, c = E.stage_math(eng.MATH_FAST_SINCOS if fn is None else fn, args.a)
    x = args.a.astype(np.float64)
    es, ec = np.abs(s.astype(np.float64) - np.sin(x)), np.abs(c.astype(np.float64) - np.cos(x))
    out = {}
    for k, name in enumerate(args.names):
        m = args.part == k
        out[name] = (float(es[m].max()), float(ec[m].max()))
        print("%s: max |error| sin %.3g cos %.3g" % (name, *out[name]))
    assert np.all(np.abs(s) <= 1.0) and np.all(np.abs(c) <= 1.0), "a sine or cosine beyond 1 (or a NaN)"
    for name, (a, b) in out.items():
        assert max(a, b) <= SURVEY_8C, (name, a, b)
        assert max(a, b) <= bound, (name, a, b)
    return out


def check_fast_atan2(E, args, bound=ATAN2_HEADER):
    r = E.stage_math(eng.MATH_FAST_ATAN2, args.a, args.b)
    y, x = args.a, args.b
    origin = (y == 0) & (x == 0)
    # exact properties.  pi here is the float nearest pi, which atan2f itself returns for (+0, -1): no float lies between it and pi
    assert not np.isnan(r).any()
    assert np.array_equal(np.signbit(r), np.signbit(y)), "fast_atan2 does not carry the sign of y"
    assert np.all(np.abs(r) <= np.float32(np.pi)), float(np.abs(r).max())
    assert origin.sum() >= 4 and np.all(r[origin] == 0), r[origin]
    # numpy's arctan2 follows C for (+-0, -0): +-pi.  fast_atan2 returns +-0 there by design (the asserts above); everywhere else the error counts
    err = np.abs(r.astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    err[origin] = 0.0
    out = {}
    for k, name in enumerate(args.names):
        m = args.part == k
        out[name] = float(err[m].max())
        print("%s: max |error| atan2 %.3g rad" % (name, out[name]))
    for name, e in out.items():
        assert e <= SURVEY_8C, (name, e)
        assert e <= bound, (name, e)
    return out
