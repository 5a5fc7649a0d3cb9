"""Input sets and requests for the checks of the fused float32 half-band (csrc/halfband_raw.h) through nrsc5hip_stage_halfband_raw
(tests/halfband_checks.py), written once: small cu8 captures (numpy, fixed seeds) that reach what the synthetic receiver captures of the
end-to-end tests do not -- every byte value in every byte lane of a dword, pair sums at both ends of their range on every tap, products
next to zero -- and the list of requests every set is run with in every form: the stream start, the first symbols that load with vector
loads, every residue of the start modulo 4, a symbol that ends on the capture's last dword, each of them at every placement of the
capture in its 16-byte-aligned device buffer."""
import functools

import numpy as np

SYM_N = 2160                              # decimated samples per symbol = dwords of capture a symbol consumes
SET_DWORDS = 3 * SYM_N + 11               # raw complex sample pairs of a set: three symbols and a ragged tail
UNIFORM_SYMS = 64                         # the long run of the random-uniform set
UNIFORM_DWORDS = (UNIFORM_SYMS + 2) * SYM_N + 11
LEADS = (0, 4, 8, 12)
SET_NAMES = ("uniform", "fullscale", "const0", "const255", "i255_q0", "i0_q255", "even0_odd255", "even255_odd0", "near127",
             "ramp1", "ramp3", "ramp37", "ramp_slip")
# Q15 taps of the half-band in window order (DevTables::hb_q15: input.c:35-40 scaled by 32767 and truncated), pair i = samples (2 i, 14 - 2 i)
TAPS_Q15 = tuple(int(np.int16(np.float32(t) * np.float32(32767.0))) for t in
                 (-0.00410953676328063, 0.032919470220804214, -0.13481467962265015, 0.6062333583831787))


def _build(name):
    n = 4 * (UNIFORM_DWORDS if name == "uniform" else SET_DWORDS)
    rng = np.random.default_rng(4100 + SET_NAMES.index(name))
    if name == "uniform":
        return rng.integers(0, 256, size=n, dtype=np.uint8)
    if name == "fullscale":
        return rng.choice(np.array([0, 255], dtype=np.uint8), size=n)
    if name in ("const0", "const255"):
        return np.full(n, 0 if name == "const0" else 255, dtype=np.uint8)
    if name in ("i255_q0", "i0_q255"):
        return np.tile(np.array([255, 0] if name == "i255_q0" else [0, 255], dtype=np.uint8), n // 2)
    if name in ("even0_odd255", "even255_odd0"):
        # raw complex samples alternate between (0, 0) and (255, 255).  The four products of an output all read EVEN raw samples and its centre
        # the odd one between them, so one phase of the alternation puts every pair sum at its lowest value, the other at its highest
        a, b = (0, 255) if name == "even0_odd255" else (255, 0)
        return np.tile(np.array([a, a, b, b], dtype=np.uint8), n // 4)
    if name == "near127":
        return rng.integers(126, 129, size=n, dtype=np.uint8)
    i = np.arange(n, dtype=np.int64)
    if name == "ramp_slip":
        # a plain ramp (k i) mod 256 shows a byte lane only the 64 values of its own residue modulo 4; this one slips by one byte every 256, so that
        # every lane of a dword meets all 256 values
        return ((i + (i >> 8)) & 255).astype(np.uint8)
    return ((int(name[4:]) * i) & 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def get(name):
    """the capture's bytes (I0 Q0 I1 Q1 ...), read-only"""
    iq = _build(name)
    iq.setflags(write=False)
    return iq


def requests(name):
    """(a0, symbols) of every request made on a set, before the leads are applied: a0 = first decimated sample of the first symbol"""
    d = get(name).size // 4
    last = d - SYM_N                                           # the symbol's last output reads the capture's last dword
    req = [(0, 2),                                             # stream start: the whole a0 < 7 branch, then a symbol behind it
           (1, 1), (3, 1), (6, 1), (7, 1), (8, 1),             # history shrinking to nothing; 7 = the first symbol on vector loads, dword 0 first
           (SYM_N - 3, 1), (SYM_N - 2, 1), (SYM_N - 1, 1), (SYM_N, 1),   # four consecutive starts: every residue modulo 4
           (last, 1)]
    if name == "uniform":
        req.append((SYM_N + 5, UNIFORM_SYMS))
    assert all(0 <= a and a + n * SYM_N <= d for a, n in req) and {a % 4 for a, _ in req[6:10]} == {0, 1, 2, 3}
    return req


def pair_byte_sums(iq):
    """[outputs, tap, component]: byte + byte of the two raw samples tap i multiplies, outputs 7 .. (the ones with no history in them).
    The kernels subtract 254 from it: s = x'_(2i) + x'_(14 - 2i), x' = byte - 127, runs from -254 to +256."""
    e = iq.reshape(-1, 4)[:, :2].astype(np.int64)              # even raw samples: the low half of every dword
    m = np.arange(7, e.shape[0])
    return np.stack([e[m - 7 + i] + e[m - i] for i in range(4)], axis=1)


def model(iq, rounding):
    """The device forms' chain acc <- acc + R(s t_i / 512) with another rounding R in place of the floor ("floor", "nearest" = ties to
    even, "trunc" = toward zero), no history: int64 [dwords, 2].  In float64 every term is exact (|s| < 2^9, |t_i| < 2^15, / 2^9)."""
    raw = np.concatenate([np.full((14, 2), 127, dtype=np.int64), iq.astype(np.int64).reshape(-1, 2)]) - 127
    m = np.arange(iq.size // 4)
    r = {"floor": np.floor, "nearest": np.rint, "trunc": np.trunc}[rounding]
    acc = 64 * raw[2 * m + 7]
    for i in range(4):
        s = raw[2 * m + 2 * i] + raw[2 * m + 14 - 2 * i]
        acc = acc + r(s.astype(np.float64) * TAPS_Q15[i] / 512.0).astype(np.int64)
    return acc
