"""Exact checks of what sits between the soft bits and the trellis, and behind it, through the nrsc5hip_stage_* hooks that run the PRODUCTION
device code on caller data -- shared by tests/test_fec_stage_cpu.py (the CPU-emulated twin) and tests/test_gpu_fec_stage.py (the gfx950 code):

  stage_p1_deint          k_p1_deint with tb.deint_lut                                       = oracle.deinterleave_p1
  stage_pids              tb.pids_gather, pids_decode_wave (trellis, descramble, CRC flag)   = deinterleave_pids, viterbi_k7, descramble, pids_crc_ok
  stage_px_interleave     k_px_deint + k_px_commit with tb.px_delay_*                        = interleave_px, its state kept from pair to pair
  stage_am_deinterleave   k_am_interleave with tb.am_deint_* and the 3-frame delay ring      = am_deinterleave, its delay lines kept from frame to frame
  stage_p1_frame          k_p1_forward / _fix / the traceback in both forms: count, descramble = bit_errors_k7, descramble
  stage_am_epilogue       am_bit_errors (carried puncture phase), am_descramble (tail mask)  = bit_errors, descramble

Every comparison is bit for bit; there is no tolerance anywhere.  The end-to-end tests cannot see a defect here: a Viterbi decoder sits behind
every permutation and corrects a few wrong trellis inputs per frame, and the BER record is compared with an absolute tolerance of 2e-5, seven
P1 disagreements.

If one of these checks finds a difference: the twins are the functions the whole-path oracle itself calls (oracle/nrsc5_oracle.c: P1 and PIDS
de-interleave, decode, descramble and count in its block step, interleave_px in px_push; oracle/nrsc5_oracle_am.c: am_deinterleave, bit_errors,
descramble in its frame decode), and the golden fixtures under tests/golden/ pin that path to the unmodified reference.  Read the mismatch --
the index planes name the wrong source cell -- against the reference's decode.c to decide which side is wrong."""
import functools

import numpy as np

from nrsc5_amd import engine as eng
from tests import fec_args as fa

EINVAL = -1
_ORACLE = None


def make_engine(lib):
    return eng.Engine(max_streams=1, q15_capacity=2 * 71280, am_enable=True, lib_path=lib)


def _use(oracle):
    global _ORACLE
    _ORACLE = oracle


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _first(bad):
    return int(np.flatnonzero(np.asarray(bad).reshape(-1))[0])


# ---- P1 de-interleave --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_p1_deint(which):
    pms = fa.pm_planes() if which == "planes" else fa.pm_random()[None]
    return _ro(np.stack([_ORACLE.deinterleave_p1(pm) for pm in pms]))


def ref_p1_deint(oracle, which):
    """int8 [3 or 1, 438528]: the twin's output for the index planes / the random matrices"""
    _use(oracle)
    return _ref_p1_deint(which)


def check_p1_deint(E, oracle, which):
    exp = ref_p1_deint(oracle, which)
    pms = fa.pm_planes() if which == "planes" else fa.pm_random()[None]
    got = np.stack([E.stage_p1_deint(pm) for pm in pms])                       # uint32 [., 146176]
    assert not (got >> 24).any(), "byte 3 of dword %d is not zero" % _first(got >> 24)
    by = np.stack([(got >> (8 * t)) & 255 for t in range(3)], axis=2).astype(np.uint8).view(np.int8).reshape(got.shape[0], -1)
    if which == "planes":
        gi, ei = fa.ids_of(by), fa.ids_of(exp)
        bad = gi != ei
        assert not bad.any(), "%d trellis inputs read another cell; first: input %d (step %d, byte %d) reads cell %d, the reference reads %d (0 = punctured)" % (
            bad.sum(), _first(bad), _first(bad) // 3, _first(bad) % 3, gi[_first(bad)] - 1, ei[_first(bad)] - 1)
    assert np.array_equal(by, exp)                                             # all 438528 positions, the punctured zeros among them
    return by.size


# ---- PIDS --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_pids(which, bc):
    pms = fa.pm_planes() if which == "planes" else (fa.pm_random() if which == "random" else fa.pm_encoded()[0])[None]
    out = []
    for pm in pms:
        coded = _ORACLE.deinterleave_pids(pm, bc)
        bits = _ORACLE.descramble(_ORACLE.viterbi_k7(coded))
        out.append((coded, bits, int(_ORACLE.pids_crc_ok(bits))))
    return out


def check_pids(E, oracle, which, bc):
    """gathered bytes, descrambled bits and CRC flag of block bc; -> the CRC flags seen"""
    _use(oracle)
    pms = fa.pm_planes() if which == "planes" else (fa.pm_random() if which == "random" else fa.pm_encoded()[0])[None]
    exp = _ref_pids(which, bc)
    got = [E.stage_pids(pm, bc) for pm in pms]
    if which == "planes":
        gi, ei = fa.ids_of([g[0] for g in got]), fa.ids_of([x[0] for x in exp])
        bad = gi != ei
        assert not bad.any(), "block %d: trellis input %d reads cell %d, the reference reads %d (0 = punctured)" % (bc, _first(bad), gi[_first(bad)] - 1, ei[_first(bad)] - 1)
    for (gc, gb, gok), (ec, eb, eok) in zip(got, exp):
        assert np.array_equal(gc, ec), (bc, _first(gc != ec))
        assert np.array_equal(gb, eb), (bc, _first(gb != eb))
        assert gok == eok, (bc, gok, eok)
    if which == "encoded":
        assert np.array_equal(got[0][1], fa.pm_encoded()[1][bc]) and got[0][2] == (0 if bc in (3, 12) else 1)
    return [g[2] for g in got]


# ---- interleaver IV ------------------------------------------------------------------------------------------------------------------------
def _px_twin(pairs):
    """[PX_PAIRS, 2, 2 L] -> (out [PX_PAIRS, 2, 3 L], ready [PX_PAIRS]) through one persistent twin state per channel"""
    n, _, two_l = pairs.shape
    out, ready, st = np.zeros((n, 2, 3 * (two_l // 2)), dtype=np.int8), np.zeros(n, dtype=np.int32), [None, None]
    for p in range(n):
        r = [0, 0]
        for ch in range(2):
            out[p, ch], r[ch], st[ch] = _ORACLE.interleave_px(pairs[p, ch], two_l // 2, st[ch])
        assert r[0] == r[1]
        ready[p] = r[0]
    return out, ready


@functools.lru_cache(maxsize=None)
def _ref_px(which, length):
    sets = fa.px_planes(length) if which == "planes" else fa.px_random(length)[None]
    res = [_px_twin(s) for s in sets]
    return _ro(np.stack([r[0] for r in res]), np.stack([r[1] for r in res]))


def ref_px(oracle, which, length):
    _use(oracle)
    return _ref_px(which, length)


def check_px(E, oracle, which, length):
    exp, exp_ready = ref_px(oracle, which, length)
    sets = fa.px_planes(length) if which == "planes" else fa.px_random(length)[None]
    res = [E.stage_px_interleave(length, s) for s in sets]
    got, ready = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    # the memory of 32 blocks wraps at pair 17 (and again at pair 33): nothing is ready before
    want_ready = (np.arange(fa.PX_PAIRS) >= 16).astype(np.int32)
    assert all(np.array_equal(r, want_ready) for r in ready), ready
    assert np.array_equal(ready, exp_ready)
    if which == "planes":
        gi, ei = fa.ids_of(got), fa.ids_of(exp)
        bad = gi != ei
        if bad.any():
            k = _first(bad)
            p, ch, o = np.unravel_index(k, gi.shape)
            raise AssertionError("length %d: %d outputs read another cell; first: pair %d channel %d output %d reads (pair, channel, position) %s, the reference %s" % (
                length, bad.sum(), p, ch, o, fa.px_cell(gi[p, ch, o], length) if gi[p, ch, o] else None, fa.px_cell(ei[p, ch, o], length) if ei[p, ch, o] else None))
    assert np.array_equal(got, exp)
    return got.size


# ---- AM interleaver_ma1 ----------------------------------------------------------------------------------------------------------------------
def _am_twin(psmi, frames):
    q, v1, v3 = None, [], []
    for f in frames:
        a, b, q = _ORACLE.am_deinterleave(psmi, f[0], f[1], f[2], f[3], queues=q)
        v1.append(a); v3.append(b)
    return np.stack(v1), np.stack(v3)


@functools.lru_cache(maxsize=None)
def _ref_am(which, psmi):
    return _ro(*_am_twin(psmi, fa.am_planes() if which == "planes" else fa.am_random()))


def ref_am(oracle, which, psmi):
    _use(oracle)
    return _ref_am(which, psmi)


def check_am(E, oracle, which, psmi):
    e1, e3 = ref_am(oracle, which, psmi)
    frames = fa.am_planes() if which == "planes" else fa.am_random()
    g1, g3 = E.stage_am_deinterleave(psmi, frames)
    assert g3.shape[1] == (90000 if psmi == fa.MA3 else 72000)
    for name, g, x in (("P1", g1, e1), ("P3", g3, e3)):
        if which == "planes":
            (gi, gd), (ei, ed) = fa.am_ids_of(g), fa.am_ids_of(x)
            bad = (gi != ei) | (gd != ed)
            if bad.any():
                k = _first(bad)
                raise AssertionError("service mode %d, %s: %d trellis inputs read another bit; first: input %d reads (matrix, cell, bit) %s%s, the reference %s%s" % (
                    psmi, name, bad.sum(), k, fa.am_bit(gi[k]) if gi[k] else None, " delayed" if gd[k] else "", fa.am_bit(ei[k]) if ei[k] else None, " delayed" if ed[k] else ""))
            # a delayed input shows the fresh ring for three frames: what frame f wrote emerges in frame f + 3
            assert (g[:3][:, gd] == -1).all()
        assert np.array_equal(g, x), (psmi, name, _first(g != x))
    return g1.size + g3.size


# ---- P1 frame: error count and descramble -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_p1_frame(name):
    soft = fa.p1_frame(name)
    scrambled = _ORACLE.viterbi_k7(soft)
    return _ro(scrambled), _ro(_ORACLE.descramble(scrambled)), int(_ORACLE.bit_errors_k7(soft, scrambled))


def ref_p1_frame(oracle, name):
    """-> (the twin decoder's bits, the same descrambled, the twin's count)"""
    _use(oracle)
    return _ref_p1_frame(name)


def check_p1_frame(E, oracle, name, walk, segments):
    scrambled, exp_bits, exp_count = ref_p1_frame(oracle, name)
    E.tune(eng.TUNE_FWD_SEGMENTS, segments)
    try:
        bits, count = E.stage_p1_frame(fa.p1_frame(name), walk)
    finally:
        E.tune(eng.TUNE_FWD_SEGMENTS, 0)
    assert np.array_equal(bits, exp_bits), "frame %s walk %d segments %d: %d bits differ, first %d" % (name, walk, segments, (bits != exp_bits).sum(), _first(bits != exp_bits))
    print("frame %s walk %d segments %d: count %d, twin %d" % (name, walk, segments, count, exp_count))
    assert count == exp_count
    if name == "codeword":
        assert np.array_equal(scrambled, fa.p1_codeword()[0])                  # the frame decodes to its code word ...
        assert count == fa.p1_codeword_expected()                              # ... so the count is known from the construction
    return count


# ---- AM frame epilogue -------------------------------------------------------------------------------------------------------------------------
def check_am_epilogue(E, oracle, length, code, kind, threads):
    soft, bits, constructed = fa.am_frame(length, code, kind)
    exp_count = oracle.bit_errors(soft, bits, 9, fa.AM_GENS[code], fa.AM_PUNCT[code].astype(np.uint8))
    exp_bits = oracle.descramble(bits)
    count, out, words = E.stage_am_epilogue(soft, bits, length, code, threads)
    print("AM frame %d code %d %s, %d work-items: count %d, twin %d" % (length, code, kind, threads, count, exp_count))
    assert count == exp_count
    if constructed is not None:
        assert count == constructed
    assert np.array_equal(out, exp_bits), _first(out != exp_bits)
    # the packed words are the same bits, and what the last word holds beyond the frame is cleared (3750: bits 6..31)
    packed = np.packbits(np.concatenate([exp_bits, np.zeros(-length % 32, dtype=np.uint8)]), bitorder="little").view(np.uint32)
    assert np.array_equal(words, packed), _first(words != packed)
    if length % 32:
        assert int(words[-1]) >> (length % 32) == 0
    return count


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------------
def check_rejections(E):
    """NRSC5HIP_EINVAL for a null pointer, an unsupported length, a count below 1, an unknown mode -- and the engine works afterwards"""
    L, h = E.lib, E._h
    pm, soft = fa.pm_random(), fa.p1_frame("zero")
    u32 = np.zeros(fa.P1_LEN, dtype=np.uint32)
    bits = np.zeros(fa.P1_LEN, dtype=np.uint8)
    one = np.zeros(4, dtype=np.int32)
    p = lambda a: a.ctypes.data
    # 1 p1_deint
    assert L.nrsc5hip_stage_p1_deint(h, None, p(u32)) == EINVAL
    assert L.nrsc5hip_stage_p1_deint(h, p(pm), None) == EINVAL
    assert L.nrsc5hip_stage_p1_deint(None, p(pm), p(u32)) == EINVAL
    # 2 p1_frame
    for args in ((None, 1, p(bits), p(one)), (p(soft), 1, None, p(one)), (p(soft), 1, p(bits), None), (p(soft), 2, p(bits), p(one)), (p(soft), -1, p(bits), p(one))):
        assert L.nrsc5hip_stage_p1_frame(h, *args) == EINVAL, args
    # 3 pids
    c240, b80 = np.zeros(240, dtype=np.int8), np.zeros(80, dtype=np.uint8)
    for args in ((None, 0, p(c240), p(b80), p(one)), (p(pm), 0, None, p(b80), p(one)), (p(pm), 0, p(c240), None, p(one)), (p(pm), 0, p(c240), p(b80), None),
                 (p(pm), 16, p(c240), p(b80), p(one)), (p(pm), -1, p(c240), p(b80), p(one))):
        assert L.nrsc5hip_stage_pids(h, *args) == EINVAL, args
    # 4 px_interleave
    pairs, out, ready = fa.px_random(2304)[:2], np.zeros((2, 2, 3 * 2304), dtype=np.int8), np.zeros(2, dtype=np.int32)
    for args in ((2304, 2, None, p(out), p(ready)), (2304, 2, p(pairs), None, p(ready)), (2304, 2, p(pairs), p(out), None),
                 (2305, 2, p(pairs), p(out), p(ready)), (0, 2, p(pairs), p(out), p(ready)), (9216, 2, p(pairs), p(out), p(ready)),
                 (2304, 0, p(pairs), p(out), p(ready)), (2304, -3, p(pairs), p(out), p(ready))):
        assert L.nrsc5hip_stage_px_interleave(h, *args) == EINVAL, args
    # 5 am_deinterleave
    sym, v1, v3 = fa.am_random()[:1], np.zeros(90000, dtype=np.int8), np.zeros(90000, dtype=np.int8)
    for args in ((fa.MA1, 1, None, p(v1), p(v3)), (fa.MA1, 1, p(sym), None, p(v3)), (fa.MA1, 1, p(sym), p(v1), None),
                 (0, 1, p(sym), p(v1), p(v3)), (3, 1, p(sym), p(v1), p(v3)), (fa.MA3, 0, p(sym), p(v1), p(v3))):
        assert L.nrsc5hip_stage_am_deinterleave(h, *args) == EINVAL, args
    # 6 am_epilogue
    s3, b, w = np.zeros(3 * 30000, dtype=np.int8), np.zeros(30000, dtype=np.uint8), np.zeros(938, dtype=np.uint32)
    ok = (p(s3), p(b), 3750, fa.E1, 64, p(one), p(b), p(w))
    for k in (0, 1, 5, 6, 7):
        assert L.nrsc5hip_stage_am_epilogue(h, *[None if i == k else a for i, a in enumerate(ok)]) == EINVAL, k
    for length, code, threads in ((3750, fa.E2, 64), (24000, fa.E1, 64), (30000, fa.E2, 64), (3751, fa.E1, 64), (0, fa.E1, 64), (3750, 0, 64), (3750, 3, 64),
                                  (3750, fa.E1, 128), (3750, fa.E1, 0), (3750, fa.E1, 1024)):
        assert L.nrsc5hip_stage_am_epilogue(h, p(s3), p(b), length, code, threads, p(one), p(b), p(w)) == EINVAL, (length, code, threads)
    # nothing was disturbed: the hooks still answer
    assert E.stage_am_epilogue(*fa.am_frame(3750, fa.E1, "random")[:2], 3750, fa.E1)[0] >= 0
    assert E.stage_pids(pm, 0)[2] in (0, 1)


def check_am_hook_needs_am_engine(lib):
    E = eng.Engine(max_streams=1, q15_capacity=2 * 71280, lib_path=lib)
    try:
        sym, v = fa.am_random()[:1], np.zeros(90000, dtype=np.int8)
        assert E.lib.nrsc5hip_stage_am_deinterleave(E._h, fa.MA1, 1, sym.ctypes.data, v.ctypes.data, v.ctypes.data) == EINVAL
    finally:
        E.close()


# ---- what the input sets hold, and what the interleaver definitions imply (no device involved) ----------------------------------------------------
def check_sets_pm(oracle):
    """every cell of the matrices has its own signature, and through the twin the P1 frame and the 16 PIDS frames together read every cell
    exactly once (decode.c:296-342: the interleavers tile the matrices)"""
    ids = fa.ids_of(fa.pm_planes())
    assert np.array_equal(ids, np.arange(1, fa.PM_CELLS + 1))                  # unique, never 0
    p1 = fa.ids_of(ref_p1_deint(oracle, "planes"))
    punct = np.arange(p1.size) % 6 == 5
    assert (p1[punct] == 0).all() and (p1[~punct] > 0).all() and p1[~punct].size == fa.P1_CODED
    _use(oracle)
    pids = np.concatenate([fa.ids_of([x[0] for x in _ref_pids("planes", bc)]) for bc in range(16)])
    punct = np.arange(pids.size) % 6 == 5
    assert (pids[punct] == 0).all() and (pids[~punct] > 0).all()
    read = np.concatenate([p1[p1 > 0], pids[pids > 0]])
    assert read.size == fa.PM_CELLS and np.array_equal(np.sort(read), np.arange(1, fa.PM_CELLS + 1))
    for bc in range(16):                                                        # a block's PIDS bits lie in that block
        own = fa.ids_of([x[0] for x in _ref_pids("planes", bc)])
        own = own[own > 0] - 1
        assert own.size == 200 and (own // 23040 == bc).all()


def check_sets_px(oracle, length):
    """every (pair, channel, position) has its own signature; through the twin no cell is read twice, a channel reads its own cells only,
    every cell written in the first 20 pairs is read (the memory holds 16 pairs), and from pair 17 on every unpunctured input is a written cell"""
    assert np.array_equal(fa.ids_of(fa.px_planes(length)).reshape(-1), np.arange(1, fa.PX_PAIRS * 4 * length + 1))
    exp, ready = ref_px(oracle, "planes", length)
    ids = fa.ids_of(exp)                                                        # [PX_PAIRS, 2, 3 L]
    punct = np.isin(np.arange(3 * length) % 6, (1, 4))
    assert (ids[:, :, punct] == 0).all()
    read = ids[ids > 0]
    assert np.unique(read).size == read.size
    for ch in range(2):
        own = ids[:, ch][ids[:, ch] > 0] - 1
        assert ((own // (2 * length)) % 2 == ch).all()
    assert np.isin(np.arange(1, 20 * 4 * length + 1), read).all()
    assert (ids[16:][:, :, ~punct] > 0).all() and np.array_equal(ready[0], (np.arange(fa.PX_PAIRS) >= 16).astype(np.int32))
    src_pair = (ids - 1) // (4 * length)
    here = np.arange(fa.PX_PAIRS)[:, None, None]
    assert ((src_pair <= here) & (src_pair >= here - 16))[ids > 0].all()       # written at most 32 blocks earlier


def check_sets_am(oracle, psmi):
    """every (matrix, cell, bit) has its own signature; through the twin no bit is read twice within a frame, and the inputs that pass the
    delay ring are the main (m*) bits: 36000 of the P1 code word's 72000, and as many of an MA3 P3 code word's (none in MA1)"""
    pl = fa.am_planes()
    bits = np.unpackbits(pl[1:1 + fa.AM_ID_BITS].reshape(fa.AM_ID_BITS, -1, 1), axis=2, bitorder="little").astype(np.int64)    # [k, 4 * 6400, 8]
    ids = sum(bits[k] << k for k in range(fa.AM_ID_BITS)).reshape(-1)
    assert np.array_equal(ids, np.arange(1, 4 * fa.AM_SYMS * 8 + 1)) and (pl[0] == 0xff).all() and not pl[-3:].any()
    e1, e3 = ref_am(oracle, "planes", psmi)
    (i1, d1), (i3, d3) = fa.am_ids_of(e1), fa.am_ids_of(e3)
    n3 = 72000 if psmi == fa.MA3 else 36000
    assert (i1 > 0).sum() == 72000 and (i3 > 0).sum() == n3
    read = np.concatenate([i1[i1 > 0], i3[i3 > 0]])
    assert np.unique(read).size == read.size
    assert d1.sum() == 36000 and d3.sum() == (36000 if psmi == fa.MA3 else 0)
    assert ((i1 > 0) == (e1[0] != 0)).all() and ((i3 > 0) == (e3[0] != 0)).all()      # a punctured input is 0 in every frame, every other one +-1
