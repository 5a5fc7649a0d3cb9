"""Seeded input sets of the PSD transport tests (tests/psd_checks.py): sessions of logical frames whose audio PDUs carry, program by
program, an HDLC byte stream of AAS packets -- ID3 tags with texts that need escaping, random-port packets, broken ones -- cut across PDUs
and frames, with the events the device code can get wrong (flags and escape pairs on the 64-byte step of k_psd, on the first and last byte
of a span, across two frames) placed on purpose.  Every session is a list of pieces (nbits, lc, [frame bits]) fed in order; `texts` is what
the generator wrote, program by program, for parse_id3.

A session is described by what it holds (describe()), and tests/test_psd_stage_cpu.py asserts those descriptions and the floors."""
from __future__ import annotations

import bisect
import functools

import numpy as np

from nrsc5_amd import synth_l2

MAX_AAS_LEN = 8212
SPAN_MAX = 236                                       # la_location <= 255: 14 header bytes, 4 of two 16-bit locators, 1 of header expansion
PSD_PORTS = (0x5100, 0x5201, 0x5202, 0x5203, 0x5204, 0x5205, 0x5206, 0x5207)


# the packet builders are generators of the package (nrsc5_amd/synth_l2.py); the tests use them under these names
id3_frame, id3_tag, aas_payload, hdlc = synth_l2.id3_frame, synth_l2.id3_tag, synth_l2.aas_payload, synth_l2.hdlc


def _markers(f: bytes):
    """offsets of the escape markers inside an HDLC frame (the first 0x7D of every pair)"""
    out, i = [], 1
    while i < len(f) - 1:
        if f[i] == 0x7D:
            out.append(i)
            i += 2
        else:
            i += 1
    return out


TITLES = ("Blue ~ Train", "Tilde}~{Brace", "}}^ up", "So What", "A~B}C", "Naima }}^ take 2", "Giant Steps", "Mr. P.C. ~}", "Équinoxe", "Ça ira}")
ARTISTS = ("John Coltrane", "Miles}Davis", "Björk ~", "Charles Mingus", "Nina Simone}}^")
SHORT_BODY = b"012"
PROPS = [(w, t) for t in ("frame", "span", "step") for w in ("pair", "last", "first")]


class _StreamBuilder:
    """One program's PSD byte stream, written against the span plan of that program: bounds[type] = the stream offsets at which a span starts in a new frame
    ("frame"), a span starts ("span"), a 64-byte step of k_psd inside a span starts ("step")."""

    def __init__(self, rng, program: int, spans, met: set):
        self.rng, self.program, self.met = rng, program, met
        self.out = bytearray()
        self.texts = []                                          # (title, artist) of every intact ID3 packet written, in order
        self.total = sum(ln for _, ln in spans)
        self.bounds = {"frame": [], "span": [], "step": []}
        at, last_frame = 0, None
        for frame, ln in spans:
            if ln > 0 and at > 0:
                self.bounds["frame" if frame != last_frame else "span"].append(at)
            for k in range(64, ln, 64):
                self.bounds["step"].append(at + k)
            if ln > 0:
                last_frame = frame
            at += ln
        self.seq = int(rng.integers(0, 1000))
        self.n = 0

    def _item(self):
        rng, k = self.rng, self.n
        self.n += 1
        kind = ("id3", "rand", "id3", "bad_fcs", "rand", "proto22", "id3", "trailing", "pad", "id3_utf16", "short")[k % 11]
        self.seq += 1
        if kind in ("id3", "id3_utf16", "bad_fcs", "trailing"):
            title = TITLES[(k + 3 * self.program) % len(TITLES)] + " #%d" % k
            artist = ARTISTS[(k + self.program) % len(ARTISTS)]
            tag = id3_tag(title, artist, album="Album %d" % self.program if k % 3 == 0 else None, genre="Jazz" if k % 4 == 0 else None, utf16=kind == "id3_utf16")
            f = hdlc(aas_payload(PSD_PORTS[self.program], self.seq, tag), or_escape=k % 2 == 1, bad_fcs=kind == "bad_fcs", trailing_escape=kind == "trailing")
            if kind in ("id3", "id3_utf16"):
                self.texts.append((title, artist))
            return f
        if kind == "rand":
            data = rng.integers(0, 256, size=int(rng.integers(60, 401)), dtype=np.uint8).tobytes()
            return hdlc(aas_payload(int(rng.integers(0x401, 0x5000)), self.seq, data), or_escape=k % 4 == 1)
        if kind == "short":                                      # protocol byte + 0..3 bytes, FCS good: shorter than port + seq (dropped as wrong protocol, a deviation)
            return hdlc(bytes([0x21]) + SHORT_BODY[:(self.program + k // 11) % 4])
        if kind == "proto22":
            return hdlc(aas_payload(PSD_PORTS[self.program], self.seq, id3_tag("not a packet", "nobody"), protocol=0x22))
        return b"\x7e\x7e\x7e"

    def _pad_for(self, f: bytes):
        """flag bytes in front of f (at most 64) that put one of its events on a bound: a kind no item of the session has hit yet first, then, for every third item, any"""
        cur = len(self.out)
        marks = _markers(f)
        for prop in [p for p in PROPS if p not in self.met] + [p for p in PROPS if p in self.met and self.n % 3 == 0]:
            what, typ = prop
            if what == "pair" and not marks:
                continue
            q = marks[len(marks) // 2] + 1 if what == "pair" else len(f) if what == "last" else 0     # the byte that must sit AT the bound
            b = self.bounds[typ]
            i = bisect.bisect_left(b, cur + q)
            if i < len(b) and b[i] - q - cur <= 64:
                self.met.add(prop)
                return b[i] - q - cur
        return 0

    def build(self) -> bytes:
        while len(self.out) < self.total:
            f = self._item()
            self.out += b"\x7e" * self._pad_for(f) + f
        return bytes(self.out[:self.total])


def _pdu(rng, room, program, stream_id, psd, nop=2, seq=0, pdu_seq=0, fill=False):
    hef = synth_l2.hef_bytes(prog_num=program) if program else b""
    return synth_l2.make_pdu(rng, room, nop=nop, codec_mode=0, stream_id=stream_id, seq=seq, pdu_seq=pdu_seq, hef=hef, psd=psd, fill=fill)


def _session_from_plan(rng, plan, rooms, to_bits=None, fill=False):
    """plan: [(nbits, lc, [[(program, stream_id, span_len), ...] per frame])] -> pieces, texts, spans (per frame: [(program, bytes)]); to_bits(frame number, PDU
    bytes, nbits) -> the frame's bits (default: zero padding, audio-only PCI)"""
    per_prog = {}
    fi = 0
    for nbits, lc, frames in plan:
        for pdus in frames:
            for program, _, ln in pdus:
                per_prog.setdefault(program, []).append((fi, ln))
            fi += 1
    met = set()
    streams, texts = {}, {}
    for program in sorted(per_prog):
        sb = _StreamBuilder(rng, program, per_prog[program], met)
        streams[program] = sb.build()
        texts[program] = sb.texts
    pos = dict.fromkeys(per_prog, 0)
    pieces, spans = [], []
    fi = 0
    for nbits, lc, frames in plan:
        bits = []
        for pdus in frames:
            body, sp = b"", []
            for k, (program, sid, ln) in enumerate(pdus):
                psd = streams[program][pos[program]:pos[program] + ln]
                pos[program] += ln
                sp.append((program, psd))
                body += _pdu(rng, rooms[nbits], program, sid, psd, nop=2, seq=(7 * fi + k) % 64, pdu_seq=fi % 8, fill=fill)
            bits.append(to_bits(fi, body, nbits) if to_bits else synth_l2.frame_from_bytes(body, nbits))
            spans.append(sp)
            fi += 1
        pieces.append((nbits, lc, bits))
    return {"pieces": pieces, "texts": texts, "spans": spans, "streams": streams}


DENSE_PROGRAMS = (0, 1, 2, 5, 7)
SPECIAL_SPANS = (0, 1, 63, 64, 65, 128, SPAN_MAX)


@functools.lru_cache(maxsize=None)
def dense(seed: int):
    """5 P1 frames x 12 PDUs over programs 0, 1, 2, 5, 7; program 2 also travels on stream_id 1; spans of every special length, the rest near the maximum"""
    rng = np.random.default_rng(9000 + seed)
    frames, k = [], 0
    for fi in range(5):
        pdus = []
        for q in range(12):
            program = DENSE_PROGRAMS[(q + fi) % 5]
            sid = 1 if program == 2 and q % 2 == 1 else 0
            ln = SPECIAL_SPANS[k % 7] if (k % 4 == 1) else int(rng.integers(180, SPAN_MAX + 1))
            pdus.append((program, sid, ln))
            k += 1
        frames.append(pdus)
    s = _session_from_plan(rng, [(146176, 0, frames)], {146176: 1500})
    s["name"] = "dense%d" % seed
    return s


DENSE_SEEDS = (1, 2, 3)
OVERFLOW_LENGTHS = (8211, 8212, 8213, 8300)


@functools.lru_cache(maxsize=None)
def overflow(raw_len: int):
    """one program, 3 P1 frames of 16 PDUs x 220 bytes: a frame of raw_len raw bytes (no escapes, FCS good), then a good packet"""
    rng = np.random.default_rng(raw_len)
    while True:
        data = rng.choice(np.array([b for b in range(256) if b not in (0x7D, 0x7E)], dtype=np.uint8), size=raw_len - 7).tobytes()
        big = hdlc(aas_payload(0x0777, 7, data))
        if len(big) == raw_len + 2:                              # no FCS byte needed an escape
            break
    good = hdlc(aas_payload(0x5100, 8, id3_tag("after the flood", "nobody")))
    stream = big + good
    total = 3 * 16 * 220
    stream = stream + b"\x7e" * (total - len(stream))
    frames, pos = [], 0
    bits = []
    for fi in range(3):
        body = b""
        for q in range(16):
            body += _pdu(rng, 1100, 0, 0, stream[pos:pos + 220], nop=2, seq=(fi * 16 + q) % 64, pdu_seq=fi)
            pos += 220
        bits.append(synth_l2.frame_from_bytes(body, 146176))
    return {"name": "overflow%d" % raw_len, "pieces": [(146176, 0, bits)], "texts": {0: [("after the flood", "nobody")]},
            "expect": [(0, 0x0777, 7, data)] * (raw_len <= MAX_AAS_LEN) + [(0, 0x5100, 8, id3_tag("after the flood", "nobody"))],
            "expect_overflows": int(raw_len > MAX_AAS_LEN)}


@functools.lru_cache(maxsize=None)
def am():
    """the 24000-bit AM form (MA1 P3 frames): 6 frames of two PDUs, programs 0 and 1"""
    rng = np.random.default_rng(24000)
    frames = [[(0, 0, int(rng.integers(100, SPAN_MAX + 1))), (1, 0, SPECIAL_SPANS[fi % 7] if fi % 2 else SPAN_MAX)] for fi in range(6)]
    s = _session_from_plan(rng, [(24000, 1, frames)], {24000: 1400})
    s["name"] = "am"
    return s


@functools.lru_cache(maxsize=None)
def p3_shared():
    """P1 frames (two PDUs, programs 0 and 1) and 4608-bit P3 frames (one PDU, program 1 then 0) in turn: the programs' states are shared by the logical channels"""
    rng = np.random.default_rng(4608)
    plan = []
    for fi in range(8):
        if fi % 2 == 0:
            plan.append((146176, 0, [[(0, 0, int(rng.integers(150, SPAN_MAX + 1))), (1, 0, int(rng.integers(150, SPAN_MAX + 1)))]]))
        else:
            plan.append((4608, 1, [[((fi // 2 + 1) % 2, 0, int(rng.integers(120, 200)))]]))
    s = _session_from_plan(rng, plan, {146176: 1500, 4608: 570})
    s["name"] = "p3_shared"
    return s


@functools.lru_cache(maxsize=None)
def fixed():
    """synth_l2.fixed_data_session's frames (sync byte 0x88, a CCC message announcing one sub-channel of 4000 bytes, five PDUs over programs 0, 1, 2) with PSD in
    every PDU: the cut moves from length - 1 to length - 17 to length - 4017 and then drops the last PDUs, and with them their part of the programs' streams"""
    rng = np.random.default_rng(7100)
    nbits, n_frames, sub_len, sync_byte, width = 146176, 7, 4000, 0x88, 16
    n = synth_l2.pdu_bytes_of(nbits)
    msg = synth_l2.hdlc_frame(bytes([0x00]) + (0).to_bytes(2, "little") + sub_len.to_bytes(2, "little"))
    ccc = b"\x7e" * (3 * width - 4) + msg + b"\x7e" * 128

    def to_bits(fi, body, nbits):
        body = bytearray(body + bytes(n - len(body)))
        body[n - 1] = sync_byte
        body[n - 1 - width:n - 1] = ccc[fi * width:(fi + 1) * width]
        return synth_l2.frame_from_bytes(bytes(body), nbits, pci=synth_l2.PCI_AUDIO_FIXED if fi % 2 == 0 else synth_l2.PCI_AUDIO_FIXED_OPP)

    frames = [[(k % 3, 0, int(rng.integers(150, SPAN_MAX + 1))) for k in range(5)] for _ in range(n_frames)]
    s = _session_from_plan(rng, [(nbits, 0, frames)], {nbits: n // 5}, to_bits, fill=True)   # PDUs that fill the frame: the last ones lie behind the cut
    s["name"] = "fixed"
    return s


_BY_NAME = {**{"dense%d" % s: functools.partial(dense, s) for s in DENSE_SEEDS},
            **{"overflow%d" % n: functools.partial(overflow, n) for n in OVERFLOW_LENGTHS},
            "am": am, "p3_shared": p3_shared, "fixed": fixed}
SESSION_NAMES = tuple(_BY_NAME)


def session(name: str):
    return _BY_NAME[name]()


def describe(s) -> dict:
    """what a session built by _session_from_plan holds, from its spans alone: the span lengths, and which events -- the second byte of an escape pair ("pair"),
    a flag as the last byte in front of ("last") or the first byte at ("first") -- fall on which bounds: the first span of a program in a new frame ("frame"), any
    other span start ("span"), a 64-byte step inside a span ("step")"""
    lens, hits = set(), set()
    tail = {}                                                    # program -> (its last byte was an escape marker, ... a flag, frame of that span)
    for fi, sp in enumerate(s["spans"]):
        for program, psd in sp:
            lens.add(len(psd))
            if not psd:
                continue
            marker = False
            if program in tail:
                marker, flag, prev_frame = tail[program]
                typ = "frame" if prev_frame != fi else "span"
                if marker:
                    hits.add(("pair", typ))
                if flag:
                    hits.add(("last", typ))
                if psd[0] == 0x7E:
                    hits.add(("first", typ))
            for i, b in enumerate(psd):
                was = marker
                marker = b == 0x7D and not was
                if i and i % 64 == 0:
                    if was:
                        hits.add(("pair", "step"))
                    if b == 0x7E:
                        hits.add(("first", "step"))
                    if psd[i - 1] == 0x7E:
                        hits.add(("last", "step"))
            tail[program] = (marker, psd[-1] == 0x7E, fi)
    return {"lens": lens, "hits": hits}
