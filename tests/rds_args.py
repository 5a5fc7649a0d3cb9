"""Seeded inputs of the RDS tests (tests/rds_checks.py): cs16 hosts at 744 187.5 S/s from nrsc5_amd/synth_fm.py with an RDS subcarrier, each
asserted to hold what it is named for, with the float64 model's run (tests/rds_model.py) computed once per input and shared; and the bit strings
of the group-level checks.  A session is N = 480 000 input samples: five timing windows (759 bits), of which the three-block sync takes the
first group and six whole groups follow -- the shortest that carries a whole name.

Exactness.  s_w and every bit of the library must equal the model's.  That can only be asked where no decision hangs on float32 rounding, so
every input asserts here, on the CPU, that each decision metric |Re(y_i conj y_{i-1})| exceeds tol (|y_i| + |y_{i-1}|) + tol^2 and each gap
between the two largest window energies exceeds twice the energy bound, tol = 4 x the largest |float32 model - float64 model| of y on that
input (the bound rds_checks holds the library's y to) and the energy bound the larger of 4 x the largest difference of the energies and
152 (2 max|y| tol + tol^2).  No bit and no window is excluded.  An input on which the two models agree to the last bit (silence) has nothing
to assert: every quantity is then exactly zero on any float32 path."""
import functools

import numpy as np

from nrsc5_amd import synth_fm as sf
from tests import fm_args as fa, rds_model as rm

N = 480000
AMP = 8000.0
PI_A, PI_B, PI_C = 0x3AAB, 0x54A9, 0x1234
CLOCK = (60310, 13, 37, -14)


def schedule(pi: int, ps: str, text: str = "Hi!", clock=CLOCK):
    """six groups: the name, one RadioText segment ended by 0x0D, the clock"""
    return sf.rds_groups(pi, ps, text=text, clock=clock, pty=5, tp=1)


AUDIO = dict(left=[(1000.0, 0.3)], right=[(2500.0, 0.2)], preemph_us=75)
# name -> transmitter arguments (None: silence)
CASES = {
    "stereo": dict(AUDIO, rds=dict(groups=schedule(PI_A, "KEXP-FM "), dev_hz=2000.0)),
    "phase90": dict(AUDIO, pilot_ppm=100.0, rds=dict(groups=schedule(PI_B, "WAAB 1  "), dev_hz=2000.0, phase=np.pi / 2)),
    "mono": dict(left=[(1000.0, 0.3)], right=[(1000.0, 0.3)], pilot=None, preemph_us=75, rds=dict(groups=schedule(PI_C, "MONO AM "), dev_hz=2000.0)),
    "wrap70": dict(AUDIO, rds=dict(groups=schedule(PI_A, "WRAP 7-0"), dev_hz=2000.0, clock_ppm=-400.0, bit_offset=0.40)),
    "wrap07": dict(AUDIO, rds=dict(groups=schedule(PI_A, "WRAP 0-7"), dev_hz=2000.0, clock_ppm=400.0, bit_offset=0.72)),
    "weak": dict(AUDIO, cnr_db=30.0, seed=30, rds=dict(groups=schedule(PI_A, "WEAK 1K "), dev_hz=1000.0)),
    "nords": dict(AUDIO, cnr_db=25.0, seed=7),
    "zero": None,
}
WITH_RDS = [k for k, v in CASES.items() if v is not None and "rds" in v]
MULTI = {1: ["stereo"], 3: ["stereo", "nords", "mono"], 9: ["stereo", "phase90", "mono", "wrap70", "wrap07", "weak", "nords", "zero", "stereo"]}


@functools.lru_cache(maxsize=None)
def host(name: str) -> np.ndarray:
    """int16 [N, 2], read-only"""
    tx = CASES[name]
    x = np.zeros((N, 2), dtype=np.int16) if tx is None else sf.fm_host(N, **{"amp": AMP, **tx})
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tables():
    tab = rm.design_taps().astype(np.float32)
    tab.setflags(write=False)
    return fa.tables()[0], tab


def sent_bits(name: str, n: int) -> np.ndarray:
    r = CASES[name]["rds"]
    return sf.RdsSignal(r["groups"], sf.PILOT_HZ, 0.0).bits(n)


def analyse(x: np.ndarray, what: str) -> dict:
    """the float64 model's run of a cs16 stream, with the bounds the float32 model gives ("tol_y", "tol_e") and the smallest margins; asserts
    that no decision hangs on float32 rounding"""
    ha, tab = tables()
    ref = rm.receive(x, ha, tab)
    r32 = rm.receive(x, ha, tab, dtype=np.float32)
    ref["err_y"] = float(np.max(np.abs(r32["y"].astype(np.complex128) - ref["y"])))
    ref["err_e"] = float(np.max(np.abs(r32["energy"].astype(np.float64) - ref["energy"])))
    tol = ref["tol_y"] = 4 * ref["err_y"]
    ymax = float(np.max(np.abs(ref["y"])))
    ref["tol_e"] = 4 * ref["err_e"]
    bound_e = max(ref["tol_e"], rm.WIN_BITS * (2 * ymax * tol + tol * tol))
    ref["margin_bit"] = ref["margin_e"] = np.inf
    if tol > 0:
        for w in range(len(ref["bits"])):
            top = np.sort(ref["energy"][w])[::-1]
            ref["margin_e"] = min(ref["margin_e"], float((top[0] - top[1]) / (2 * bound_e)))
            assert top[0] - top[1] > 2 * bound_e, (what, w, top[:2], bound_e)
        mags = _point_magnitudes(ref)
        for w in range(len(ref["bits"])):
            need = tol * mags[w] + tol * tol
            ratio = np.abs(ref["metric"][w]) / need
            ref["margin_bit"] = min(ref["margin_bit"], float(ratio.min()))
            assert np.all(np.abs(ref["metric"][w]) > need), (what, w, float(ratio.min()))
        assert np.array_equal(r32["stream"], ref["stream"]) and np.array_equal(r32["s"], ref["s"])
    else:
        assert not ref["y"].any() and not ref["stream"].any()
    return ref


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """analyse() of the named input, read-only; asserts what the input is named for"""
    ref = analyse(host(name), name)
    assert len(ref["bits"]) == 5 and ref["stream"].size in (758, 759, 760), (name, ref["stream"].size)
    _assert_named(name, ref)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _point_magnitudes(ref):
    """|y_i| + |y_{i-1}| of every decision, window by window, from the sampling points the model's s_w and seam rule give"""
    y, s = ref["y"], ref["s"]
    out, last = [], None
    for w in range(len(s)):
        pts = [w * rm.WIN_PTS + rm.S * k + int(s[w]) for k in range(rm.WIN_BITS)]
        if w > 0:
            gap = rm.S + int(s[w]) - int(s[w - 1])
            if gap < 4:
                pts = pts[1:]
            elif gap > 12:
                pts = [last + rm.S] + pts
        prev = ([last] if last is not None else pts[:1]) + pts[:-1]
        if last is None:
            pts, prev = pts[1:], prev[1:]
        out.append(np.abs(y[np.array(pts)]) + np.abs(y[np.array(prev)]))
        last = pts[-1]
    return out


def _assert_named(name: str, ref: dict):
    tx = CASES[name]
    g = ref["groups"]
    s = [int(v) for v in ref["s"]]
    if tx is None:
        assert not g.events and g.stats["syncs_gained"] == 0
        return
    if "rds" not in tx:
        assert not g.events and g.stats["syncs_gained"] == 0 and not g.synced          # the model never syncs
        return
    # the source's bits come back: the stream is the sent one from its second bit on (the first point has no predecessor), or from a neighbour of
    # that one where bit_offset moves the first sampling point; the first decision may still lean on the zeros in front of the stream
    n = ref["stream"].size
    errors = min(int(np.sum(sent_bits(name, n + 3)[lag + 1:lag + n] != ref["stream"][1:])) for lag in (0, 1, 2))
    if name == "weak":
        assert tx["rds"]["dev_hz"] == 1000.0 and tx["cnr_db"] == 30.0
    assert errors == 0, (name, errors)
    snap = g.snapshot()
    assert snap["pi"] == tx["rds"]["groups"][0][0] and snap["synced"] == 1 and g.stats["groups"] == 6 and g.stats["groups_dropped"] == 0
    assert snap["ps"] is not None and snap["rt"] == b"Hi!\r" and snap["clock"] == CLOCK
    assert [e["kind"] for e in g.events] == ["pi", "rt", "clock", "ps"], [e["kind"] for e in g.events]
    if name == "wrap70":
        assert any(a == 7 and b == 0 for a, b in zip(s, s[1:])), s
        assert (g.stats["seam_drops"], g.stats["seam_inserts"]) == (1, 0)
    elif name == "wrap07":
        assert any(a == 0 and b == 7 for a, b in zip(s, s[1:])), s
        assert (g.stats["seam_drops"], g.stats["seam_inserts"]) == (0, 1)
    else:
        assert g.stats["seam_drops"] == 0 and g.stats["seam_inserts"] == 0 and max(s) - min(s) <= 1, s    # (+100 ppm moves the clock 0.6 grid steps)
    if name == "mono":
        assert tx["pilot"] is None
    if name == "phase90":
        assert tx["pilot_ppm"] == 100.0 and tx["rds"]["phase"] == np.pi / 2


# ------------------------------------------------------------------------------------------------------------------- group level
def corrupt(bits: np.ndarray, flips=(), delete=(), insert=()) -> np.ndarray:
    out = np.array(bits, dtype=np.uint8)
    for p in flips:
        out[p] ^= 1
    keep = np.ones(out.size, bool)
    keep[list(delete)] = False
    out = out[keep]
    for p in sorted(insert, reverse=True):
        out = np.insert(out, p, 1)
    return out


def long_schedule():
    """0A, 0B, 2A, 2B, 4A and several uncounted types; a PI change; an A/B flag toggle; a text ended by 0x0D and one of all 16 segments; a clock
    with a negative offset"""
    g = sf.rds_groups(PI_A, "KEXP-FM ", text="Now playing: a song", clock=(60310, 23, 59, -9), pty=5, tp=1)
    g += sf.rds_groups(PI_A, "KEXP-FM ", text="x" * 61 + "END", ab=1)                                   # flag toggle, all 16 segments
    g += [(PI_A, 1 << 12 | 0x15, 0x1111, 0x2222), (PI_A, 3 << 12 | 1 << 11, PI_A, 0x3333), (PI_A, 8 << 12, 1, 2), (PI_A, 14 << 12 | 1 << 11, PI_A, 7),
          (PI_A, 15 << 12, 0xABCD, 0xEF01)]
    g += sf.rds_groups(PI_A, "KEXP 0B ", text="two bytes per segment", version_b=True, ab=1)             # 0B, 2B
    g += sf.rds_groups(PI_B, "WAAB HD ", text="after the PI change", clock=(60311, 0, 1, 4), ab=0)       # PI change
    g += sf.rds_groups(PI_B, "WAAB HD ", text="after the PI change")                                     # nothing new: no event
    return g


@functools.lru_cache(maxsize=None)
def group_cases() -> dict:
    """name -> (bits, reset_at or None, raw groups, correct_burst)"""
    base = sf.rds_bits(long_schedule())
    short = sf.rds_bits(schedule(PI_A, "KEXP-FM ") * 3)
    rng = np.random.default_rng(26)
    cases = {"schedule": (base, None, False, 2), "schedule_raw": (base, None, True, 2)}
    # a single-bit error and a 2-bit burst in every block position: one block of every group from the third on
    flips1 = [104 * (2 + p) + 26 * (p % 4) + p for p in range(26)]
    flips2 = [q for p in range(25) for q in (flips1[p], flips1[p] + 1)]
    many = base
    cases["single_bit_errors"] = (corrupt(many, flips1), None, False, 2)
    cases["burst2_errors"] = (corrupt(many, flips2), None, False, 2)
    cases["burst2_with_burst1"] = (corrupt(many, flips2), None, False, 1)
    cases["errors_with_burst0"] = (corrupt(many, flips1), None, False, 0)
    cases["burst3"] = (corrupt(short, [104 * 3 + 30, 104 * 3 + 31, 104 * 3 + 32]), None, False, 2)
    cases["deleted_bit"] = (corrupt(np.tile(short, 3), delete=[104 * 5 + 40]), None, False, 2)
    cases["inserted_bit"] = (corrupt(np.tile(short, 3), insert=[104 * 5 + 40]), None, False, 2)
    cases["noise_in_front"] = (np.concatenate([rng.integers(0, 2, 64).astype(np.uint8), short]), None, False, 2)
    cases["reset_inside"] = (np.tile(short, 2), short.size + 17, False, 2)
    cases["reset_at_end"] = (short, short.size, False, 2)
    cases["random"] = (np.random.default_rng(200000).integers(0, 2, 200000).astype(np.uint8), None, False, 2)
    for v in cases.values():
        v[0].setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def group_reference(name: str):
    """the model on a group-level case -> the Groups object; asserts what the case is named for"""
    bits, rst, raw, burst = group_cases()[name]
    g = rm.Groups(burst, raw)
    if rst is None:
        g.push(bits)
    else:
        g.push(bits[:rst])
        g.reset()
        g.events = []                                                     # (the events in front of the reset were delivered; the checks compare what follows)
        g.push(bits[rst:])
    st, kinds = g.stats, [e["kind"] for e in g.events]
    if name in ("schedule", "schedule_raw"):
        for t in ("g0A", "g0B", "g2A", "g2B", "g4A", "g1A", "g3B", "g8A", "g14B", "g15A"):
            assert st[t] > 0, t
        assert sum(e["kind"] == "pi" for e in g.events) == 2 and sum(e["kind"] == "clock" for e in g.events) == 2
        texts = [e["data"] for e in g.events if e["kind"] == "rt"]
        assert b"Now playing: a song\r" in texts and b"x" * 61 + b"END" in texts and b"two bytes per segment\r" in texts, texts
        assert any(e["kind"] == "clock" and e["v"][3] == -9 for e in g.events)
        assert st["groups_dropped"] == 0 and st["blocks_invalid"] == 0 and (kinds.count("group") == st["groups"]) == raw
    elif name == "single_bit_errors":
        assert st["blocks_corrected"] == 26 and st["blocks_invalid"] == 0 and st["groups_dropped"] == 0
    elif name == "burst2_errors":
        assert st["blocks_corrected"] == 25 and st["blocks_invalid"] == 0 and st["groups_dropped"] == 0
    elif name == "burst2_with_burst1":
        assert st["blocks_corrected"] == 0 and st["blocks_invalid"] == 25 and st["groups_dropped"] == 25
    elif name == "errors_with_burst0":
        assert st["blocks_corrected"] == 0 and st["blocks_invalid"] == 26 and st["groups_dropped"] == 26 and st["syncs_lost"] == 0
    elif name == "burst3":
        assert st["blocks_invalid"] == 1 and st["groups_dropped"] == 1 and st["syncs_lost"] == 0
    elif name in ("deleted_bit", "inserted_bit"):
        assert st["syncs_lost"] == 1 and st["syncs_gained"] == 2 and g.synced and st["blocks_invalid"] >= 16
    elif name == "noise_in_front":
        assert st["syncs_gained"] == 1 and g.snapshot()["ps"] == b"KEXP-FM "
    elif name == "reset_inside":
        assert g.nbits == bits.size - rst and g.snapshot()["ps"] == b"KEXP-FM "
    elif name == "reset_at_end":
        assert g.nbits == 0 and g.pi == -1 and not g.events
    elif name == "random":
        assert st["syncs_gained"] == 0 and not g.events                    # 200 000 seeded random bits: the model reports no sync
    return g
