"""Argument sets for the checks of csrc/fastmath.h (tests/math_checks.py), written once: deterministic (numpy, fixed seeds), built from
named parts so that a failure names the neighbourhood it fell into, and shuffled by a fixed permutation before they reach a kernel -- the
parts are branch by branch, a wave must not be.

Sizes: 2^20 arguments per function on the device and a 2^16 subset for the CPU-emulated build (parts of up to 1024 arguments whole, the
others thinned evenly).  ref_atan2f's set is 2^22: its ratio-threshold part alone -- 6 thresholds x 2048 x x 65 neighbouring y x 4 sign
quadrants -- is 3.2 million pairs, and every pair of it is kept."""
import functools

import numpy as np

N_DEVICE = 1 << 20
N_DEVICE_ATAN2F = 1 << 22
N_EMU = 1 << 16
F32, U32 = np.float32, np.uint32


class ArgSet:
    """a (and b): the arguments in the order a kernel gets them; part[i] indexes names"""

    def __init__(self, parts, seed):
        names, a, b, ids = [], [], [], []
        for k, (name, v) in enumerate(parts):
            va, vb = v if isinstance(v, tuple) else (v, None)
            assert va.ndim == 1 and (vb is None or vb.shape == va.shape), name
            names.append(name); a.append(va); ids.append(np.full(va.size, k, dtype=np.int16))
            if vb is not None:
                b.append(vb)
        assert not b or len(b) == len(a)
        perm = np.random.default_rng(seed).permutation(sum(v.size for v in a))
        self.names = names
        self.a = np.ascontiguousarray(np.concatenate(a)[perm])
        self.b = np.ascontiguousarray(np.concatenate(b)[perm]) if b else None
        self.part = np.concatenate(ids)[perm]

    def __len__(self):
        return self.a.size

    def _take(self, idx):
        out = object.__new__(ArgSet)
        out.names, out.a, out.part = self.names, np.ascontiguousarray(self.a[idx]), self.part[idx]
        out.b = None if self.b is None else np.ascontiguousarray(self.b[idx])
        return out

    def subset(self, n=N_EMU, whole=1024):
        """parts of at most `whole` arguments entirely, every n_big / room-th argument of the others (the order is already a random one)"""
        counts = np.bincount(self.part, minlength=len(self.names))
        small = counts <= whole
        room = n - int(counts[small].sum())
        big = np.flatnonzero(~small[self.part])
        assert room > 0
        keep = big[np.unique(np.linspace(0, big.size - 1, min(room, big.size)).astype(np.int64))]
        return self._take(np.sort(np.concatenate([np.flatnonzero(small[self.part]), keep])))

    def only(self, *names):
        ks = [self.names.index(n) for n in names]
        return self._take(np.flatnonzero(np.isin(self.part, ks)))

    def part_name(self, i):
        return self.names[int(self.part[i])]


def bits(v):
    return np.ascontiguousarray(v, dtype=F32).view(U32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=U32).view(F32)


def neighbours(mag, k):
    """mag: positive finite floats [n] -> [n][2 k + 1]: the floats k below ... k above each, by bit pattern"""
    u = bits(mag).astype(np.int64)[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]
    assert u.min() > 0 and u.max() < 0x7f800000
    return from_bits(u.astype(U32).reshape(-1)).reshape(u.shape)


def _uniform(rng, n, scale):
    return ((rng.random(n) * 2 - 1) * scale).astype(F32)


def _raw(rng, n):
    return from_bits(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(U32))


def _signed(rng, mag):
    return np.where(rng.integers(0, 2, size=mag.shape) == 1, -mag, mag).astype(F32)


def _log_uniform(rng, n, e_lo, e_hi):
    """positive normal floats: biased exponent uniform in [e_lo, e_hi], random mantissa"""
    e = rng.integers(e_lo, e_hi + 1, size=n, dtype=np.uint64)
    return from_bits(((e << 23) | rng.integers(0, 1 << 23, size=n, dtype=np.uint64)).astype(U32))


# ---- sincosf ---------------------------------------------------------------------------------------------------------------------
SINCOSF_SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-40, -1e-40, 3.4e38, -3.4e38, 0.78539816, 0.78539822, 120.0, 119.99999,
                             2.4414062e-4, 2.4414059e-4, 3.14159274, -3.14159274, 6.28318548, 1.57079637, 1e9, 16777216.0], dtype=F32)   # tests/test_ref_sincosf.py
SINCOSF_TOPS = (0x398, 0x3f4, 0x42f, 0x7f8)                  # abstop12 thresholds of ref_sincosf: 2^-12, 0.75 (the top 12 bits of pi/4), 120, inf
HALF_PI = 1.5707963267948966


@functools.lru_cache(maxsize=None)
def sincosf_args():
    rng = np.random.default_rng(1101)
    parts = []
    # 64 floats on either side of every branch threshold (bit pattern top << 20), both signs; behind 0x7f8 they are NaNs
    for top in SINCOSF_TOPS:
        u = (np.int64(top) << 20) + np.arange(-64, 64, dtype=np.int64)
        u = np.concatenate([u, u | 0x80000000]).astype(U32)
        parts.append(("threshold 0x%03x" % top, from_bits(u)))
    # fast reduction: the quadrant n = round(y * 2 / pi) flips at (k + 1/2) pi/2
    k = np.arange(-76, 77, dtype=np.float64)
    centre = np.abs(((k + 0.5) * HALF_PI).astype(F32))
    parts.append(("quadrant flips", (neighbours(centre, 32) * np.sign(k + 0.5)[:, None].astype(F32)).reshape(-1)))
    # large reduction: every biased exponent 133 .. 254 (|y| >= 64; the branch is taken from 120 on), 512 mantissas, both signs: every idx 0..15
    # (table path: idx > 3) and every shift 0..7
    e = np.repeat(np.arange(133, 255, dtype=np.uint64), 512)
    u = (e << 23) | rng.integers(0, 1 << 23, size=e.size, dtype=np.uint64)
    parts.append(("large reduction", from_bits(np.concatenate([u, u | 0x80000000]).astype(U32))))
    parts.append(("specials", SINCOSF_SPECIALS))
    n = (N_DEVICE - sum(v.size for _, v in parts)) // 5
    parts.append(("+-6.5", _uniform(rng, n, 6.5)))
    parts.append(("+-2000", _uniform(rng, n, 2000.0)))
    parts.append(("+-0.79", _uniform(rng, n, 0.79)))
    parts.append(("raw patterns", _raw(rng, n)))
    rest = N_DEVICE - sum(v.size for _, v in parts)
    parts.append(("k pi/2 +- 1e-3", (rng.integers(-1000, 1001, size=rest) * HALF_PI + (rng.random(rest) * 2 - 1) * 1e-3).astype(F32)))
    return ArgSet(parts, seed=1)


# ---- atan2f ----------------------------------------------------------------------------------------------------------------------
ATAN2F_SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-40, -1e-40, 3.4e38, 0.4375, 0.6875, 1.1875, 2.4375, 33554432.0], dtype=F32)   # tests/test_ref_atan2f.py
ATANF_THRESHOLDS = (0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 25, 2.0 ** -29)         # ratio thresholds of ref_atanf
QUADRANTS = ((1, 1), (-1, 1), (1, -1), (-1, -1))                                    # signs of (y, x)


def _quadrants(y, x):
    return (np.concatenate([F32(sy) * y for sy, _ in QUADRANTS]), np.concatenate([F32(sx) * x for _, sx in QUADRANTS]))


@functools.lru_cache(maxsize=None)
def atan2f_args():
    rng = np.random.default_rng(707)
    parts = []
    sp = ATAN2F_SPECIALS
    parts.append(("special grid", (np.repeat(sp, sp.size), np.tile(sp, sp.size))))
    # the ratio thresholds: |y / x| within 32 floats of the threshold on either side, x of any mantissa and of magnitudes 2^-20 .. 2^20
    for thr in ATANF_THRESHOLDS:
        x = _log_uniform(rng, 2048, 127 - 20, 127 + 20)
        y = neighbours((x.astype(np.float64) * thr).astype(F32), 32)
        parts.append(("ratio %g" % thr, _quadrants(y.reshape(-1), np.repeat(x, 65))))
    # exponent differences k = (iy - ix) >> 23 of 58 .. 63 (the mantissas make it 57 .. 63) in both directions: the k > 60 and k < -60 cuts
    ys, xs = [], []
    for k in range(58, 64):
        for direction in (1, -1):
            lo = rng.integers(1, 255 - k, size=512, dtype=np.uint64)
            m = rng.integers(0, 1 << 23, size=(2, 512), dtype=np.uint64)
            small, large = from_bits(((lo << 23) | m[0]).astype(U32)), from_bits((((lo + k) << 23) | m[1]).astype(U32))
            ys.append(large if direction > 0 else small); xs.append(small if direction > 0 else large)
    parts.append(("exponent difference", _quadrants(np.concatenate(ys), np.concatenate(xs))))
    # x == 1 goes to ref_atanf directly: y of all magnitudes, and the neighbourhood of every threshold
    y1 = np.concatenate([_uniform(rng, 5120, 4.0), _raw(rng, 5120), _signed(rng, _log_uniform(rng, 5364, 127 - 40, 127 + 40)),
                         neighbours(np.array(ATANF_THRESHOLDS, dtype=F32), 32).reshape(-1), -neighbours(np.array(ATANF_THRESHOLDS, dtype=F32), 32).reshape(-1)])
    parts.append(("x == 1", (y1, np.ones_like(y1))))
    # denormals (2^14 pairs): both operands; a normal over a denormal and the other way round; normal operands whose quotient is denormal
    # (the exponents differ by 126 .. 149; a little less keeps the smallest normal quotients in) or underflows (150 and more) -- for x > 0
    # the quotient itself is the result
    den = lambda n: from_bits(rng.integers(1, 1 << 23, size=n, dtype=np.uint64).astype(U32))
    parts.append(("denormal / denormal", (_signed(rng, den(4096)), _signed(rng, den(4096)))))
    parts.append(("normal / denormal", (_signed(rng, _log_uniform(rng, 4096, 1, 254)), _signed(rng, den(4096)))))
    parts.append(("denormal / normal", (_signed(rng, den(2048)), _signed(rng, _log_uniform(rng, 2048, 1, 40)))))
    d = rng.integers(118, 161, size=6144, dtype=np.int64)
    ex = (d + 1 + (rng.random(6144) * (254 - d)).astype(np.int64)).clip(1, 254)
    xq = _log_uniform(rng, 6144, 127, 127).astype(np.float64) * 2.0 ** (ex - 127)
    yq = _log_uniform(rng, 6144, 127, 127).astype(np.float64) * 2.0 ** (ex - d - 127)
    parts.append(("denormal quotient", (_signed(rng, yq.astype(F32)), _signed(rng, xq.astype(F32)))))
    n = (N_DEVICE_ATAN2F - sum(v[0].size for _, v in parts)) // 4
    parts.append(("unit square", (_uniform(rng, n, 1.0), _uniform(rng, n, 1.0))))
    parts.append(("tall", (_uniform(rng, n, 1e3), _uniform(rng, n, 1e-3))))
    parts.append(("raw patterns", (_raw(rng, n), _raw(rng, n))))
    rest = N_DEVICE_ATAN2F - sum(v[0].size for _, v in parts)
    parts.append(("right half-plane", (_uniform(rng, rest, 50.0), (rng.random(rest) * 100).astype(F32))))
    return ArgSet(parts, seed=2)


# ---- the fast forms: the distributions of tools/probe/math_probe.hip, finite arguments only ----------------------------------------
FAST_SINCOS_RANGES = (("+-pi", 3.1415927), ("+-100", 100.0), ("+-2000", 2000.0))


def _probe_uniform(rng, n):
    """the probe's uniform: a 24-bit integer / 2^23 - 1, in float"""
    return (rng.integers(0, 1 << 24, size=n).astype(F32) / F32(8388608.0) - F32(1.0)).astype(F32)


@functools.lru_cache(maxsize=None)
def fast_sincos_args():
    rng = np.random.default_rng(31)
    n = N_DEVICE // 3
    parts = [(name, _probe_uniform(rng, n if k else N_DEVICE - 2 * n) * F32(r)) for k, (name, r) in enumerate(FAST_SINCOS_RANGES)]
    return ArgSet(parts, seed=3)


@functools.lru_cache(maxsize=None)
def fast_sincos_reduced_args():
    rng = np.random.default_rng(32)
    x = _probe_uniform(rng, N_DEVICE - 4) * F32(3.2)
    return ArgSet([("|x| <= 3.2", x), ("ends", np.array([0.0, -0.0, 3.2, -3.2], dtype=F32))], seed=4)


TAN_PI_8 = 0.41421356237309503


@functools.lru_cache(maxsize=None)
def fast_atan2_args():
    rng = np.random.default_rng(33)
    parts = []
    mag = lambda n: np.abs(_probe_uniform(rng, n)) * np.where(rng.integers(0, 4, size=n) == 0, F32(1e-3), F32(4.0)) + F32(1e-9)     # the probe's magnitudes, never 0
    zero = lambda n: _signed(rng, np.zeros(n, dtype=F32))
    m = mag(4096)
    parts.append(("y axis", (_signed(rng, m), zero(4096))))
    m = mag(4096)
    parts.append(("x axis", (zero(4096), _signed(rng, m))))
    m = mag(4096)
    parts.append(("diagonals", _quadrants(m, m)))
    mx = mag(128)
    mn = neighbours((mx.astype(np.float64) * TAN_PI_8).astype(F32), 32).reshape(-1)
    mx = np.repeat(mx, 65)
    yq, xq = _quadrants(np.concatenate([mn, mx]), np.concatenate([mx, mn]))               # all eight octants
    parts.append(("ratio tan(pi/8)", (yq, xq)))
    z = np.array([0.0, -0.0], dtype=F32)
    parts.append(("(0, 0)", (np.repeat(z, 2), np.tile(z, 2))))
    n = N_DEVICE - sum(v[0].size for _, v in parts)
    y = _probe_uniform(rng, n) * np.where(rng.integers(0, 8, size=n) == 0, F32(1e-3), F32(4.0))
    x = _probe_uniform(rng, n) * np.where(rng.integers(0, 4, size=n) == 0, F32(1e-3), F32(4.0))
    parts.append(("[-4, 4]^2", (y.astype(F32), x.astype(F32))))
    return ArgSet(parts, seed=5)


# ---- the double series -----------------------------------------------------------------------------------------------------------
def _series_args(seed, bound):
    rng = np.random.default_rng(seed)
    ends = np.array([0.0, bound, -bound, 1e-300, -1e-300], dtype=np.float64)
    x = (rng.random(N_DEVICE - ends.size) * 2 - 1) * bound
    x[::4] *= 1e-3
    return ArgSet([("|x| <= %g" % bound, x), ("ends", ends)], seed=seed)


@functools.lru_cache(maxsize=None)
def small_cos_sin_args():
    return _series_args(41, 0.25)


@functools.lru_cache(maxsize=None)
def small_atan_args():
    return _series_args(42, 0.26)


SETS = {"sincosf": sincosf_args, "atan2f": atan2f_args, "fast_sincos": fast_sincos_args, "fast_sincos_reduced": fast_sincos_reduced_args,
        "fast_atan2": fast_atan2_args, "small_cos_sin": small_cos_sin_args, "small_atan": small_atan_args}


@functools.lru_cache(maxsize=None)
def get(name, emu=False):
    """the set of one function, or its 2^16 subset for the CPU-emulated build; built once per session and never written to"""
    s = SETS[name]()
    s = s.subset() if emu else s
    for v in (s.a, s.b):
        if v is not None:
            v.setflags(write=False)
    return s
