"""EAS alerts (SAME) of an analog FM host, restated in float64 from the definition (include/nrsc5hip.h, "SAME") -- the reference
of tests/same_checks.py.  The signal path is written from the definition, not from the kernels: segment sums of the discriminator output against
the two exact phasors (np.add.reduceat over the segment starts), bit sums of eight segments, q, and feed-forward timing and decisions per window
of 64 bits.  dtype=np.float32 runs that path in float32 in the order the definition fixes (samples of a segment one after the other, the eight
segment sums in order, the metrics in the lane order and butterfly): the reference's own estimate of what float32 costs.

The framer and the vote (Framer) are plain Python over the bit stream, rule by rule as the definition lists them.  They hold the same state as
k_same_frames, so a rule misread once would be misread on both sides; what anchors them from outside are the assertions of tests/same_args.py:
the text that was sent comes back, from the signal and from hand-made bit strings."""
import numpy as np

from tests import fm_model as fm

DEN = 35721                      # mark 200 / DEN, space 150 / DEN cycles per Fs1 sample; a bit is DEN / 50 samples
K_MARK, K_SPACE = 200, 150
S = 8                            # grid points per bit
GRID = 400                       # grid point r starts at floor(35721 r / 400)
WIN_BITS = 64
WIN_PTS = WIN_BITS * S
TAIL = S - 1
TEXT_MAX = 268
VOTE_BITS = 2604
KINDS = (None, "burst", "message")
HEADER, EOM = 1, 2
STATS = ("bits", "preambles", "bursts", "bursts_aborted", "messages", "groups_no_message", "eom_messages", "seam_drops", "seam_inserts", "events")


def grid(r):
    return (DEN * r) // GRID


def segments_total(m_total: int) -> int:
    """segments that lie inside m_total samples of d"""
    return (GRID * (m_total + 1) - 1) // DEN


def windows_total(segs: int) -> int:
    return max(0, (segs - TAIL) // WIN_PTS)


LATENCY_IN = 2 * grid(WIN_PTS + TAIL) - 1       # input samples behind which window 0 is decided; window w: 2 grid(512 w + 519) - 1


def table() -> np.ndarray:
    """float64 [DEN][2]: cos, sin of 2 pi k / DEN"""
    t = 2 * np.pi * np.arange(DEN) / DEN
    return np.stack([np.cos(t), np.sin(t)], axis=1)


def tones(d: np.ndarray, tab: np.ndarray, dtype=np.float64) -> np.ndarray:
    """d [m_total] -> c complex [segments][2]: mark, space; tab as the library stores it (float32 [DEN][2])"""
    ct = np.complex128 if dtype == np.float64 else np.complex64
    nr = segments_total(d.size)
    starts = grid(np.arange(nr + 1, dtype=np.int64))
    tab = np.asarray(tab, dtype=np.float32).astype(dtype)
    out = np.zeros((nr, 2), ct)
    if nr == 0:
        return out
    m = np.arange(starts[-1], dtype=np.int64)
    x = d[:starts[-1]].astype(dtype)
    for col, k in enumerate((K_MARK, K_SPACE)):
        t = tab[(k * m) % DEN]
        if dtype == np.float64:
            out[:, col] = np.add.reduceat(x * t[:, 0], starts[:-1]) - 1j * np.add.reduceat(x * t[:, 1], starts[:-1])
            continue
        re, im = np.zeros(nr, np.float32), np.zeros(nr, np.float32)
        n = np.diff(starts)
        for i in range(int(n.max())):                       # one sample after the other, fused as the definition has it
            on = i < n
            idx = np.minimum(starts[:-1] + i, starts[-1] - 1)
            xi = x[idx].astype(np.float64)                  # fma(d, cos, re): the product of two float32 is exact in float64, one rounding of the sum
            re = np.where(on, (re.astype(np.float64) + xi * t[idx, 0].astype(np.float64)).astype(np.float32), re)
            im = np.where(on, (im.astype(np.float64) + xi * t[idx, 1].astype(np.float64)).astype(np.float32), im)
        out[:, col] = (re - 1j * im).astype(ct)
    return out


def decision_values(c: np.ndarray, dtype=np.float64) -> np.ndarray:
    """c [segments][2] -> q [segments - 7]"""
    n = c.shape[0] - TAIL
    if n <= 0:
        return np.zeros(0, dtype)
    parts = [c.real.astype(dtype), c.imag.astype(dtype)]
    sums = []
    for p in parts:
        acc = p[0:n].copy()
        for k in range(1, S):                               # added in that order
            acc = (acc + p[k:k + n]).astype(dtype)
        sums.append(acc)
    re, im = sums
    return ((re[:, 0] * re[:, 0] + im[:, 0] * im[:, 0]).astype(dtype) - (re[:, 1] * re[:, 1] + im[:, 1] * im[:, 1]).astype(dtype)).astype(dtype)


def decide(q: np.ndarray, dtype=np.float64) -> dict:
    """-> {"metric" [windows][8], "s" [windows], "bits": list per window of uint8 arrays, "value": list per window of the q the bits were cut from,
    "drops", "inserts"} for the complete windows of q"""
    nw = q.size // WIN_PTS
    metric = np.zeros((nw, S), dtype)
    s = np.zeros(nw, np.int64)
    bits, value = [], []
    drops = inserts = 0
    last = None                                             # grid index of the last sampling point
    for w in range(nw):
        a = np.abs(q[w * WIN_PTS:(w + 1) * WIN_PTS]).astype(dtype).reshape(WIN_BITS, S)
        if dtype == np.float64:
            metric[w] = a.sum(axis=0)
        else:                                               # lanes 8 g + s sum bits g, g + 8, ... in order, then a butterfly over g
            part = np.zeros((8, S), np.float32)
            for k in range(WIN_BITS // 8):
                part = (part + a[8 * k:8 * k + 8]).astype(np.float32)
            for step in (1, 2, 4):
                part = (part + part[np.arange(8) ^ step]).astype(np.float32)
            metric[w] = part[0]
        s[w] = int(np.argmax(metric[w]))                    # ties to the lowest s
        pts = [w * WIN_PTS + S * k + int(s[w]) for k in range(WIN_BITS)]
        if w > 0:
            gap = S + int(s[w]) - int(s[w - 1])
            if gap < 4:
                pts = pts[1:]
                drops += 1
            elif gap > 12:
                pts = [last + S] + pts
                inserts += 1
        v = q[np.array(pts)]
        bits.append((v > 0).astype(np.uint8))
        value.append(v)
        last = pts[-1]
    return {"metric": metric, "s": s, "bits": bits, "value": value, "drops": drops, "inserts": inserts}


class Framer:
    """framing and the three-burst vote of one station's bit stream"""

    def __init__(self, burst_events: bool = True):
        self.burst_events = burst_events
        self.events = []
        self.reset()

    def reset(self):
        self.stats = dict.fromkeys(STATS, 0)
        self.nbits = 0
        self.reg = 0                                        # the last 16 bits, the newest in bit 15
        self.state = "search"
        self.fill = 0
        self.buf = bytearray()
        self.pre_bit = self.first_bit = 0
        self.group, self.group_kind, self.group_done, self.group_last = [], 0, 0, 0
        self.msg = None                                     # (text, kind, first, last)

    def snapshot(self) -> dict:
        kinds = (None, "header", "eom")
        text, kind, first, last = self.msg if self.msg else (None, 0, -1, -1)
        return {"text": text, "kind": kinds[kind], "first": first, "last": last, "group_bursts": len(self.group),
                "group_kind": kinds[self.group_kind if self.group else 0], "in_message": int(self.state == "message")}

    def _event(self, kind: str, first: int, last: int, v, data: bytes):
        self.events.append({"kind": kind, "first": first, "last": last, "v": list(v) + [0] * (8 - len(v)), "data": bytes(data)})
        self.stats["events"] += 1

    def push(self, bits):
        for b in bits:
            self._bit(int(b) & 1)
        return self

    def _bit(self, b: int):
        idx = self.nbits
        self.nbits += 1
        self.stats["bits"] += 1
        self.reg = self.reg >> 1 | b << 15
        if self.state != "message" and idx >= 15 and self.reg == 0xABAB:
            if self.state == "search":
                self.pre_bit = idx
                self.stats["preambles"] += 1
            self.state, self.fill = "preamble", 0           # sets the byte boundary
            return
        if self.state == "search":
            return
        self.fill += 1
        if self.fill < 8:
            return
        self.fill = 0
        byte = self.reg >> 8
        if self.state == "preamble":
            if byte == 0xAB:
                return
            if byte in (ord("Z"), ord("N")):
                self.state, self.buf, self.first_bit = "message", bytearray([byte]), idx - 7
            else:
                self.state = "search"
            return
        if not 0x20 <= byte <= 0x7E:
            return self._abort()
        self.buf.append(byte)
        if len(self.buf) == 4:
            if self.buf == b"NNNN":
                return self._burst(EOM, idx)
            if self.buf != b"ZCZC":
                return self._abort()
        elif len(self.buf) > 4 and byte == ord("-"):
            tail = bytes(self.buf[4:])
            if b"+" in tail and tail[tail.index(b"+"):].count(b"-") == 3:
                return self._burst(HEADER, idx)
        if len(self.buf) >= TEXT_MAX:
            self._abort()

    def _abort(self):
        self.state = "search"
        self.stats["bursts_aborted"] += 1

    def _burst(self, kind: int, last: int):
        self.state = "search"
        self.stats["bursts"] += 1
        text, pre, first = bytes(self.buf), self.pre_bit, self.first_bit
        joins = 1 <= len(self.group) < 3 and kind == self.group_kind and pre - self.group_last <= VOTE_BITS
        if not joins:
            if self.group and self.group_done == 0:
                self.stats["groups_no_message"] += 1        # the group it closes never agreed
            self.group, self.group_done, self.group_kind = [], 0, kind
        earlier = list(self.group)
        self.group.append(text)
        self.group_last = last
        if self.burst_events:
            self._event("burst", first, last, [kind, len(self.group), first - pre], text)
        if self.group_done:
            return
        if text in earlier:
            return self._message(text, first, last)
        if len(self.group) == 3:
            a, b, c = self.group
            out = bytearray()
            ok = len(a) == len(b) == len(c)
            for x, y, z in zip(a, b, c) if ok else ():
                if x == y or x == z:
                    out.append(x)
                elif y == z:
                    out.append(y)
                else:
                    ok = False
                    break
            if ok:
                self._message(bytes(out), first, last)
            else:
                self.group_done = 2
                self.stats["groups_no_message"] += 1

    def _message(self, text: bytes, first: int, last: int):
        self.group_done = 1
        self.msg = (text, self.group_kind, first, last)
        self.stats["messages"] += 1
        if self.group_kind == EOM:
            self.stats["eom_messages"] += 1
        self._event("message", first, last, [self.group_kind, len(self.group)], text)


def receive(x: np.ndarray, ha: np.ndarray, tab: np.ndarray, dtype=np.float64) -> dict:
    """one channel, cs16 [n, 2] -> everything the checks compare: d, c, q, metric, s, bits (per window and joined), the framer"""
    d, _ = fm.front(x, np.asarray(ha, dtype=np.float32).astype(dtype), dtype)
    c = tones(d, tab, dtype)
    q = decision_values(c, dtype)
    out = decide(q, dtype)
    out["d"], out["c"], out["q"] = d, c, q
    out["stream"] = np.concatenate(out["bits"]) if out["bits"] else np.zeros(0, np.uint8)
    g = Framer().push(out["stream"])
    g.stats["seam_drops"], g.stats["seam_inserts"] = out["drops"], out["inserts"]
    out["framer"] = g
    return out
