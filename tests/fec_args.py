"""Inputs for the exact checks of the FEC stage's permutations, error counts and descramblers (tests/fec_checks.py), written once: numpy
only, fixed seeds, each the smallest input that still reaches the edge it is named for.

Permutations (P1 de-interleave, PIDS gather, interleaver IV, AM interleaver_ma1 with its delay ring)
  * index planes: three inputs whose byte at source cell c is byte 0, 1 and 2 of c + 1 (0 is left to the punctured zeros and to memory that
    was never written), so that the three outputs together name the source cell of every output; for the AM de-interleaver, whose sources
    are single bits, one L1 frame per bit of the id of (matrix, cell, bit) behind a marker frame of all ones, which tells the inputs that
    pass the 3-frame delay ring (marker in frame 3) from those that do not (frame 0);
  * random full range: every byte value, -128 included, which the receiver's soft bits never take.
Error counts and descramblers
  * P1 frames: full-range noise, the all-zero frame (every metric a tie), all 127, and a code word at +-64 with wrong signs at chosen
    places: the first six and the last six steps (the six wrapped bits of the walk form), both sides of 64-step chunk boundaries, the third
    bit of an even and of an odd (punctured) step, zeros and -128 at unpunctured places (the wrong signs of the two dense groups at the
    wrap are weak, +-16: the frame must still decode to its code word for the count to be known from the construction);
  * AM frames of every (length, code) the AM path uses: random +-1 / 0 against random bits, and code words with wrong signs at puncture
    phases 0 and plen - 1 and on both sides of the wrap."""
import functools

import numpy as np

from nrsc5_amd import synth, synth_am

PM_CELLS = 16 * 23040                     # soft bits of an L1 frame's interleaver matrices
P1_LEN, P1_CODED = 146176, 365440
PX_LENS = (2304, 4608)
PX_PAIRS = 36                             # the interleaver IV memory (32 blocks) wraps at pair 17 and again at pair 33
AM_SYMS = 6400                            # hard symbols of one partition matrix per L1 frame
AM_RANDOM_FRAMES = 6                      # two turns of the 3-slot delay ring
AM_ID_BITS = 18                           # ((matrix * 6400 + cell) * 8 + bit) + 1 < 2^18
AM_PLANE_FRAMES = 1 + AM_ID_BITS + 3      # marker, the id's bits, three frames that flush the delay ring
MA1, MA3 = 1, 2
E1, E2 = 1, 2                             # NRSC5HIP_CODE_*
AM_FRAMES = ((3750, E1), (24000, E2), (30000, E1))      # every (length, code) of decode_process_p1_p3_am (decode.c:507-554)
AM_GENS = {E1: synth_am.GENS_E1, E2: synth_am.GENS_E2}
AM_PUNCT = {E1: synth_am.PUNCT_E1, E2: synth_am.PUNCT_E2}


def _ro(a):
    a.setflags(write=False)
    return a


# ---- permutations ----------------------------------------------------------------------------------------------------------------------
def id_planes(ncells):
    """int8 [3, ncells]: plane p holds byte p of (cell + 1)"""
    ids = np.arange(1, ncells + 1, dtype=np.uint32)
    return np.stack([((ids >> (8 * p)) & 255).astype(np.uint8).view(np.int8) for p in range(3)])


def ids_of(planes_out):
    """the three outputs of a permutation run on id_planes -> the source cell + 1 of every output, 0 where nothing was read"""
    u = [np.asarray(p).view(np.uint8).astype(np.int64) for p in planes_out]
    return u[0] | u[1] << 8 | u[2] << 16


@functools.lru_cache(maxsize=None)
def pm_planes():
    return _ro(id_planes(PM_CELLS))


@functools.lru_cache(maxsize=None)
def pm_random():
    return _ro(np.random.default_rng(7301).integers(-128, 128, size=PM_CELLS, dtype=np.int8))


@functools.lru_cache(maxsize=None)
def pm_encoded():
    """an L1 frame's matrices at +-127 whose 16 PIDS frames are valid (CRC-12 good) but for blocks 3 and 12, whose CRC is broken -> (pm, the 16 frames)"""
    rng = np.random.default_rng(7302)
    pids = np.stack([synth.pids_frame_bits(rng, corrupt=bc in (3, 12)) for bc in range(16)])
    m = synth.encode_l1_frame(rng.integers(0, 2, size=P1_LEN, dtype=np.uint8), pids)
    return _ro((m.astype(np.int16) * 254 - 127).astype(np.int8)), _ro(pids)


@functools.lru_cache(maxsize=None)
def px_planes(length):
    """int8 [3, PX_PAIRS, 2, 2 * length]: cell = ((pair * 2 + channel) * 2 * length + position)"""
    return _ro(id_planes(PX_PAIRS * 2 * 2 * length).reshape(3, PX_PAIRS, 2, 2 * length))


@functools.lru_cache(maxsize=None)
def px_random(length):
    """int8 [PX_PAIRS, 2, 2 * length], full range; the two channels carry different data"""
    x = np.random.default_rng(7310 + length).integers(-128, 128, size=(PX_PAIRS, 2, 2 * length), dtype=np.int8)
    assert not np.array_equal(x[:, 0], x[:, 1])
    return _ro(x)


def px_cell(ident, length):
    """id -> (pair, channel, position)"""
    c = int(ident) - 1
    return c // (4 * length), (c // (2 * length)) % 2, c % (2 * length)


@functools.lru_cache(maxsize=None)
def am_planes():
    """uint8 [AM_PLANE_FRAMES, 4, 6400]: frame 0 all ones; in frame 1 + k bit b of cell c of matrix m is bit k of ((m * 6400 + c) * 8 + b) + 1;
    the last three frames zero"""
    ids = np.arange(1, 4 * AM_SYMS * 8 + 1, dtype=np.uint32).reshape(4, AM_SYMS, 8)
    out = np.zeros((AM_PLANE_FRAMES, 4, AM_SYMS), dtype=np.uint8)
    out[0] = 0xff
    for k in range(AM_ID_BITS):
        out[1 + k] = np.packbits(((ids >> k) & 1).astype(np.uint8), axis=2, bitorder="little")[:, :, 0]
    return _ro(out)


def am_ids_of(v):
    """outputs [AM_PLANE_FRAMES, n] of the de-interleaver on am_planes -> (id of the source bit of every output, 0 = punctured; delayed [n])"""
    v = np.asarray(v)
    direct, late = v[0] > 0, v[3] > 0
    ids = np.zeros(v.shape[1], dtype=np.int64)
    for k in range(AM_ID_BITS):
        ids |= np.where(direct, v[1 + k] > 0, np.where(late, v[4 + k] > 0, False)).astype(np.int64) << k
    return ids, late & ~direct


def am_bit(ident):
    """id -> (matrix, cell, bit)"""
    c = int(ident) - 1
    return "pl pu s t".split()[c // (8 * AM_SYMS)], (c // 8) % AM_SYMS, c % 8


@functools.lru_cache(maxsize=None)
def am_random():
    """uint8 [AM_RANDOM_FRAMES, 4, 6400], every byte value: the twin and the kernel read single bits of a symbol, so nothing is out of range"""
    return _ro(np.random.default_rng(7320).integers(0, 256, size=(AM_RANDOM_FRAMES, 4, AM_SYMS), dtype=np.uint8))


# ---- P1 frames for the error count and the descramble -----------------------------------------------------------------------------------
P1_FRAMES = ("noise", "zero", "all127", "codeword")
# (step, bit) of the code-word frame whose sign is wrong.  Chunks of the walk are 64 steps: 63 | 64, 127 | 128, 63999 | 64000 and the last
# boundary 146111 | 146112; the wrap: steps 0..5 (bit_errors_k7_at) and the last six
_K7_WRAP = [(i, i % 2) for i in range(6)] + [(P1_LEN - 6 + i, (i + 1) % 2) for i in range(6)]
_K7_CHUNKS = [(63, 0), (64, 1), (127, 1), (128, 0), (63999, 2), (64000, 2), (P1_LEN - 65, 0), (P1_LEN - 64, 0)]
K7_FLIPS = tuple(_K7_WRAP + _K7_CHUNKS + [(1000, 2), (1001, 2), (70001, 2)])      # (1000, 2): third bit of an even step; (1001, 2), (70001, 2), (63999, 2): of odd steps -- punctured
K7_ZEROS = ((2000, 0), (2001, 1), (2002, 2), (2003, 2), (90000, 0), (90001, 0), (90002, 1), (90003, 1))
K7_WEAK = 16                              # magnitude of the wrong signs in the two dense groups at the wrap: twelve consecutive steps with a wrong +-64 each are
                                          # more than the code corrects (the decoder then returns another code word and the construction says nothing about the count);
                                          # the count looks at signs only
K7_MIN_NEAR = (3000, 3001, 3002, 3004, 100000, 100001)      # -128 at the first place from these steps on whose code bit is 0 (no disagreement) ...
K7_MIN_WRONG_NEAR = (110000, 120000)                        # ... and as the wrong sign of a code bit 1


@functools.lru_cache(maxsize=None)
def p1_codeword():
    """-> (info bits [146176] (scrambled domain: what the decoder returns), code bits [146176, 3])"""
    info = np.random.default_rng(7330).integers(0, 2, size=P1_LEN, dtype=np.uint8)
    return _ro(info), _ro(synth.conv_encode_k7(info))


def _k7_min_places():
    """-> ((step, bit) holding -128 over a code bit 0, (step, bit) holding -128 over a code bit 1), unpunctured, clear of every other chosen place"""
    _, cw = p1_codeword()
    taken = set(K7_FLIPS) | set(K7_ZEROS)
    pick = lambda i0, v: next((i, j) for i in range(i0, P1_LEN) for j in range(3) if cw[i, j] == v and not (j == 2 and i % 2) and (i, j) not in taken)
    return tuple(pick(i, 0) for i in K7_MIN_NEAR), tuple(pick(i, 1) for i in K7_MIN_WRONG_NEAR)


def p1_codeword_expected():
    """disagreements the re-encode count must find in the code-word frame, from the code word alone: wrong signs at unpunctured places,
    plus zeros at unpunctured places whose code bit is 1 (a zero is not > 0)"""
    _, cw = p1_codeword()
    unp = lambda i, j: not (j == 2 and i % 2 == 1)
    n = sum(1 for i, j in K7_FLIPS + _k7_min_places()[1] if unp(i, j))
    n += sum(1 for i, j in K7_ZEROS if unp(i, j) and cw[i, j] == 1)
    return n


@functools.lru_cache(maxsize=None)
def p1_frame(name):
    """int8 [3 * 146176]"""
    if name == "noise":
        return _ro(np.random.default_rng(7331).integers(-128, 128, size=3 * P1_LEN, dtype=np.int8))
    if name == "zero":
        return _ro(np.zeros(3 * P1_LEN, dtype=np.int8))
    if name == "all127":
        return _ro(np.full(3 * P1_LEN, 127, dtype=np.int8))
    _, cw = p1_codeword()
    soft = (cw.astype(np.int16) * 128 - 64).astype(np.int8)
    for i, j in K7_FLIPS:
        soft[i, j] = -soft[i, j] if (i, j) not in _K7_WRAP else -np.sign(soft[i, j]) * K7_WEAK
    for i, j in K7_ZEROS:
        soft[i, j] = 0
    for group in _k7_min_places():
        for i, j in group:
            soft[i, j] = -128
    return _ro(soft.reshape(-1))


# ---- AM frames for am_bit_errors / am_descramble ----------------------------------------------------------------------------------------
def am_flip_places(length, code):
    """coded positions j = 3 i + q of the AM code-word frame whose sign is wrong: one per puncture phase 0 and plen - 1 early in the frame and
    late in it, and every position of the steps on both sides of the wrap (the last eight steps and the first eight: the re-encoder's window
    of nine bits straddles it)"""
    plen = len(AM_PUNCT[code])
    n = 3 * length
    first = lambda ph, lo: next(j for j in range(lo, n) if j % plen == ph)
    places = {first(0, 300), first(plen - 1, 300), first(0, n // 2), first(plen - 1, n // 2)}
    places |= set(range(0, 24)) | set(range(n - 24, n))
    return tuple(sorted(places))


@functools.lru_cache(maxsize=None)
def am_frame(length, code, kind):
    """-> (soft int8 [3 * length], bits uint8 [length], the count expected from the construction or None)"""
    rng = np.random.default_rng(7340 + length + code)
    bits = rng.integers(0, 2, size=length, dtype=np.uint8)
    if kind == "random":
        return _ro(rng.integers(-1, 2, size=3 * length, dtype=np.int8)), _ro(bits), None
    cw = synth_am.conv_encode_k9(bits, AM_GENS[code]).astype(np.int16)
    soft = (2 * cw - 1).astype(np.int8)
    places = np.array(am_flip_places(length, code))
    soft[places] = -soft[places]
    punct = np.resize(AM_PUNCT[code], 3 * length)
    return _ro(soft), _ro(bits), int(punct[places].sum())
