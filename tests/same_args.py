"""Seeded inputs of the SAME tests (tests/same_checks.py): cs16 hosts at 744 187.5 S/s from nrsc5_amd/synth_fm.py with SAME bursts in the audio,
each asserted to hold what it is named for, with the float64 model's run (tests/same_model.py) computed once per input and shared; and the bit
strings of the framer-level checks.  A session is N = 736 000 input samples: eight timing windows of 64 bits, the shortest that holds the 464
bits of a minimal header burst.

Bounds.  c, q and the metrics of the library are held to 4 x the largest |float32 model - float64 model| of the same input (tol_c, tol_q,
tol_m).  s_w must be exact, which can only be asked where no window's choice hangs on float32 rounding: every input asserts here, on the CPU,
that the two largest metrics of every window are further apart than twice that window's own bound: 4 x the largest difference of the two
models' metrics in the window plus 64 x 4 x the largest difference of their q in it (a metric is 64 values of |q|; the error of q goes with its
size, and a window of programme alone has values a thousand times below a burst's, so the session's largest error says nothing there).  Bits are
exact wherever the model's |q| exceeds tol_q; the others are counted ("weak"), and every input asserts that none of them lies inside a burst.
An input on which the two models agree to the last bit (silence) has nothing to assert: every quantity is exactly zero on any float32 path."""
import functools

import numpy as np

from nrsc5_amd import synth_fm as sf
from tests import fm_args as fa, same_model as sm

N = 736000
N_SHORT = 368000                           # four windows: what the chunking checks push in thousands of pieces
AMP = 8000.0
T_BIT = 1.0 / sf.SAME_BIT_HZ
DELAY_S = 56.5 / sf.FS                     # d[m] is the frequency at input sample 2 m - 56.5: the channel filter's delay and the difference
HEADER = "ZCZC-WXR-TOR-029095+0030-1231405-KXYZ/FM -"         # the shortest header there is: one location, 42 bytes
LONG = "ZCZC-WXR-TOR-029095-029097+0030-1231405-KXYZ/FM -"
EOM = "NNNN"
PROGRAMME = dict(left=[(1000.0, 0.2)], right=[(3000.0, 0.1)])


def at_bits(b: float) -> float:
    """start time of a burst whose first bit begins b bit periods into the receiver's grid"""
    return b * T_BIT + DELAY_S


def _same(start_bits, text, **kw):
    return dict(bursts=[(at_bits(start_bits), text)], level=0.3, **kw)


# name -> transmitter arguments (None: silence)
CASES = {
    "eom": dict(PROGRAMME, same=_same(20.0, EOM)),
    "header": dict(PROGRAMME, same=_same(2.0, HEADER)),
    **{"eighth%d" % k: dict(PROGRAMME, same=_same(31.0 + k / 8.0, EOM)) for k in range(8)},
    "seam": dict(PROGRAMME, same=_same(64.0, EOM)),
    "ppm_plus": dict(PROGRAMME, same=dict(bursts=[((2 + 0.9375) * T_BIT, HEADER)], level=0.3, clock_ppm=50.0)),
    "ppm_minus": dict(PROGRAMME, same=dict(bursts=[((2 + 0.875) * T_BIT, HEADER)], level=0.3, clock_ppm=-50.0)),
    "preemph": dict(PROGRAMME, preemph_us=75, same=_same(2.0, HEADER)),
    "cnr30": dict(PROGRAMME, cnr_db=30.0, seed=30, same=_same(2.0, HEADER)),
    "programme": dict(left=[(1000.0, 0.3)], right=[(3000.0, 0.2)], preemph_us=75),
    "zero": None,
}
WITH_BURST = [k for k, v in CASES.items() if v is not None and "same" in v]
MULTI = {1: ["header"], 3: ["header", "programme", "eom"], 9: ["header", "eom", "seam", "ppm_plus", "ppm_minus", "preemph", "cnr30", "zero", "eighth3"]}


@functools.lru_cache(maxsize=None)
def host(name: str) -> np.ndarray:
    """int16 [N, 2], read-only"""
    tx = CASES[name]
    x = np.zeros((N, 2), dtype=np.int16) if tx is None else sf.fm_host(N, **{"amp": AMP, **tx})
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tables():
    tab = sm.table().astype(np.float32)
    tab.setflags(write=False)
    return fa.tables()[0], tab


def sent(name: str):
    """-> (text, the burst's bits) of a case with a burst"""
    text = CASES[name]["same"]["bursts"][0][1]
    return text, sf.same_bits(text)


def analyse(x: np.ndarray, what: str) -> dict:
    """the float64 model's run of a cs16 stream, with the bounds the float32 model gives (tol_c, tol_q, tol_m), the smallest margin of the timing and
    "weak": per window the places whose |q| is within tol_q; asserts that no window's timing hangs on float32 rounding"""
    ha, tab = tables()
    ref = sm.receive(x, ha, tab)
    r32 = sm.receive(x, ha, tab, dtype=np.float32)
    ref["tol_c"] = 4 * float(np.max(np.abs(r32["c"].astype(np.complex128) - ref["c"])))
    ref["tol_q"] = 4 * float(np.max(np.abs(r32["q"].astype(np.float64) - ref["q"])))
    ref["tol_m"] = 4 * float(np.max(np.abs(r32["metric"].astype(np.float64) - ref["metric"])))
    ref["margin_m"] = np.inf
    if ref["tol_c"] > 0:
        for w in range(len(ref["bits"])):
            win = slice(w * sm.WIN_PTS, (w + 1) * sm.WIN_PTS)
            bound_m = 4 * float(np.max(np.abs(r32["metric"][w].astype(np.float64) - ref["metric"][w]))) + \
                sm.WIN_BITS * 4 * float(np.max(np.abs(r32["q"][win].astype(np.float64) - ref["q"][win])))
            top = np.sort(ref["metric"][w])[::-1]
            ref["margin_m"] = min(ref["margin_m"], float((top[0] - top[1]) / (2 * bound_m)))
            assert top[0] - top[1] > 2 * bound_m, (what, w, top[:2], bound_m)
        assert np.array_equal(r32["s"], ref["s"])
    else:
        assert not ref["c"].any() and not ref["q"].any() and not ref["stream"].any()
    ref["weak"] = [np.abs(v) <= ref["tol_q"] for v in ref["value"]]
    return ref


def burst_span(ref: dict):
    """-> (first, last) index in the model's bit stream of the burst it framed, preamble included; None without one"""
    ev = [e for e in ref["framer"].events if e["kind"] == "burst"]
    if not ev:
        return None
    return ev[0]["first"] - 128, ev[0]["last"]


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """analyse() of the named input, read-only; asserts what the input is named for"""
    ref = analyse(host(name), name)
    assert len(ref["bits"]) == 8 and 510 <= ref["stream"].size <= 514, (name, ref["stream"].size)
    _assert_named(name, ref)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference_short(name: str) -> dict:
    """analyse() of the first N_SHORT samples of the named input"""
    ref = analyse(host(name)[:N_SHORT], name)
    assert len(ref["bits"]) == 4
    return ref


def _assert_named(name: str, ref: dict):
    tx = CASES[name]
    g = ref["framer"]
    s = [int(v) for v in ref["s"]]
    if tx is None:
        assert not g.events and g.stats["preambles"] == 0 and not ref["stream"].any()        # d = 0 throughout: all-zero bits
        return
    if "same" not in tx:
        assert not g.events and g.stats["preambles"] == 0 and g.stats["bits"] >= 510          # a 1 kHz + 3 kHz programme: zero events
        assert tx["left"][0][0] == 1000.0 and tx["right"][0][0] == 3000.0
        return
    text, bits = sent(name)
    kinds = [(e["kind"], e["data"]) for e in g.events]
    assert kinds == [("burst", text.encode())], (name, kinds)                                 # one burst: no message yet
    assert g.stats["bursts"] == 1 and g.stats["bursts_aborted"] == 0 and g.stats["preambles"] == 1
    a, b = burst_span(ref)
    # every bit of the burst, the preamble's first included, is the sent one, and none is weak
    got = ref["stream"][a:b + 1]
    assert got.size == bits.size and np.array_equal(got, bits), name
    weak = np.concatenate(ref["weak"])
    assert not weak[a:b + 1].any(), (name, int(weak[a:b + 1].sum()))
    snap = g.snapshot()
    assert snap["text"] is None and snap["group_bursts"] == 1 and snap["group_kind"] == ("eom" if text == EOM else "header")
    wa, wb = a // sm.WIN_BITS, b // sm.WIN_BITS                                               # (within a bit or two: the seams move the count)
    if name.startswith("eighth"):
        k = int(name[6:])
        assert abs(tx["same"]["bursts"][0][0] - DELAY_S - (31.0 + k / 8.0) * T_BIT) < 1e-12
    if name == "seam":
        assert 64 - 2 <= a <= 64 + 1, a                                                       # the burst begins where window 1 does
    if name in ("ppm_plus", "ppm_minus"):
        assert abs(tx["same"]["clock_ppm"]) == 50.0
        inside = s[wa:wb + 1]
        assert any(p == 7 and n == 0 for p, n in zip(inside, inside[1:])) and any(p == 0 and n == 7 for p, n in zip(inside, inside[1:])), s
        assert g.stats["seam_drops"] >= 1 and g.stats["seam_inserts"] >= 1                    # both rules fire inside the burst
    if name == "preemph":
        assert tx["preemph_us"] == 75
    if name == "cnr30":
        assert tx["cnr_db"] == 30.0
    if name in ("header", "preemph", "cnr30"):
        assert len(text) == 42 and g.stats["seam_drops"] == 0 and g.stats["seam_inserts"] == 0


# ------------------------------------------------------------------------------------------------------------------- framer level
def gap(n: int) -> np.ndarray:
    return np.zeros(n, dtype=np.uint8)


def train(texts, gaps=48, lead=24) -> np.ndarray:
    """bursts with `gaps` zero bits between them (one number or a list), `lead` zeros in front and 24 behind"""
    gaps = [gaps] * (len(texts) - 1) if np.isscalar(gaps) else list(gaps)
    out = [gap(lead)]
    for i, t in enumerate(texts):
        out.append(sf.same_bits(t))
        out.append(gap(gaps[i] if i < len(gaps) else 24))
    return np.concatenate(out)


def _swap(text: str, at: int, ch: str) -> str:
    assert text[at] != ch
    return text[:at] + ch + text[at + 1:]


JOIN_GAP = sm.VOTE_BITS - 16                # zeros between two bursts whose second preamble match lies 2604 bits behind the first's last bit


@functools.lru_cache(maxsize=None)
def frame_cases() -> dict:
    """name -> (bits, reset_at or None)"""
    h = sf.same_bits(HEADER)
    cases = {
        "slip_in_preamble": np.concatenate([gap(24), np.delete(h, 43), gap(24)]),
        "nonprintable": train([_swap(HEADER, 10, "\x07")]),
        "wrong_first_four": train([_swap(HEADER, 3, "X"), "NNNX"]),
        "long_268": train(["ZCZC-" + "A" * 300]),
        "two_of_three": train([HEADER, _swap(HEADER, 12, "X"), HEADER]),
        "two_equal_at_once": train([HEADER, HEADER, HEADER]),
        "majority": train([_swap(LONG, 5, "C"), _swap(LONG, 20, "7"), _swap(LONG, 40, "Q")]),
        "disagree": train([_swap(LONG, 20, "1"), _swap(LONG, 20, "2"), _swap(LONG, 20, "3")]),
        "unequal_lengths": train([HEADER, LONG, _swap(LONG, 5, "C")]),
        "gap_2604": train([HEADER, HEADER], gaps=JOIN_GAP),
        "gap_2605": train([HEADER, HEADER], gaps=JOIN_GAP + 1),
        "header_then_eom": train([HEADER] * 3 + [EOM] * 3, gaps=520),
        "reset_inside": train([HEADER, HEADER, HEADER]),
        "reset_at_end": train([HEADER, HEADER]),
        "random": np.random.default_rng(3125).integers(0, 2, 100000).astype(np.uint8),
    }
    out = {}
    for k, v in cases.items():
        v.setflags(write=False)
        rst = None
        if k == "reset_inside":
            rst = 24 + h.size + 48 + 200                    # inside the second burst's text: the third is alone in its group
        elif k == "reset_at_end":
            rst = v.size
        out[k] = (v, rst)
    return out


@functools.lru_cache(maxsize=None)
def frame_reference(name: str):
    """the model on a framer-level case -> the Framer; asserts what the case is named for"""
    bits, rst = frame_cases()[name]
    g = sm.Framer()
    if rst is None:
        g.push(bits)
    else:
        g.push(bits[:rst])
        g.reset()
        g.events = []                                                     # (the events in front of the reset were delivered; the checks compare what follows)
        g.push(bits[rst:])
    st = g.stats
    kinds = [e["kind"] for e in g.events]
    msgs = [e["data"] for e in g.events if e["kind"] == "message"]
    if name == "slip_in_preamble":
        assert kinds == ["burst"] and g.events[0]["data"] == HEADER.encode() and st["preambles"] == 2     # back to search, and found again
    elif name == "nonprintable":
        assert not kinds and st["bursts_aborted"] == 1 and st["preambles"] == 1
    elif name == "wrong_first_four":
        assert not kinds and st["bursts_aborted"] == 2 and st["preambles"] == 2
    elif name == "long_268":
        assert not kinds and st["bursts_aborted"] == 1 and g.snapshot()["in_message"] == 0
    elif name == "two_of_three":
        assert kinds == ["burst", "burst", "burst", "message"] and msgs == [HEADER.encode()] and g.events[-1]["v"][:2] == [sm.HEADER, 3]
    elif name == "two_equal_at_once":
        assert kinds == ["burst", "burst", "message", "burst"] and msgs == [HEADER.encode()] and st["messages"] == 1
    elif name == "majority":
        assert kinds == ["burst", "burst", "burst", "message"] and msgs == [LONG.encode()] and LONG.encode() not in [e["data"] for e in g.events[:3]]
    elif name == "disagree":
        assert kinds == ["burst"] * 3 and st["groups_no_message"] == 1 and st["messages"] == 0
    elif name == "unequal_lengths":
        assert kinds == ["burst"] * 3 and st["groups_no_message"] == 1 and st["messages"] == 0
    elif name == "gap_2604":
        assert g.events[1]["first"] - 113 - g.events[0]["last"] == sm.VOTE_BITS and kinds == ["burst", "burst", "message"]
    elif name == "gap_2605":
        assert g.events[1]["first"] - 113 - g.events[0]["last"] == sm.VOTE_BITS + 1 and kinds == ["burst", "burst"] and st["groups_no_message"] == 1
        assert g.events[1]["v"][1] == 1                                     # it opened a group of its own
    elif name == "header_then_eom":
        assert msgs == [HEADER.encode(), b"NNNN"] and st["eom_messages"] == 1 and st["messages"] == 2 and st["bursts"] == 6
        assert g.snapshot()["kind"] == "eom" and g.snapshot()["group_bursts"] == 3
    elif name == "reset_inside":
        assert kinds == ["burst"] and g.events[0]["v"][1] == 1 and g.nbits == bits.size - rst
    elif name == "reset_at_end":
        assert g.nbits == 0 and not g.events and g.snapshot()["text"] is None
    elif name == "random":
        assert not g.events and st["bursts"] == 0                           # 100 000 seeded random bits: no burst
    return g
