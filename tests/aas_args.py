"""Seeded packet lists of the data-service tests (tests/aas_checks.py): AAS packets (port, seq, data) as output_aas_push takes them -- a Station Information
Guide, LOT fragments with and without headers, stream and packet data, PSD-port packets in between -- with the cases the device code can get wrong placed
on purpose.  A list is {"packets", "lot_files", "ref": the reference is well defined on it}; tests/test_aas_stage_cpu.py asserts on the model's output
alone that every list holds what it is named for."""
from __future__ import annotations

import functools

import numpy as np

from nrsc5_amd import synth_l2

SIG_PORT = 0x20
LOT_PORT, STREAM_PORT, PACKET_PORT, ODD_PORT, LOT_PORT_B = 0x1000, 0x1001, 0x1002, 0x1003, 0x1100
MIME_LOGO, MIME_ART, MIME_TEXT = 0xD9C72536, 0xBE4B7536, 0xBB492AAC
EXPIRY = (2031 - 1900, 4, 17, 21, 59)                            # tm_year, tm_mon, tm_mday, tm_hour, tm_min


# the packet builders are generators of the package (nrsc5_amd/synth_l2.py); the tests use them under these names
sig_service, sig_name, sig_data, sig_audio = synth_l2.sig_service, synth_l2.sig_name, synth_l2.sig_data, synth_l2.sig_audio
expiry_word, lot_header, lot_packet = synth_l2.lot_expiry, synth_l2.lot_header, synth_l2.lot_packet


def psd_packet(program: int, seq: int, n: int):
    """a PSD-port packet with n data bytes (an ID3 tag cut to n bytes, or padded)"""
    tag = synth_l2.id3_tag("Title %d" % seq, "Artist %d" % program)
    return (0x5100 if program == 0 else 0x5200 + program, seq, (tag + bytes(n))[:n], program)


STANDARD_SIG = (sig_service(1, audio=True) + sig_name(b"MPS") + sig_audio(0, 0, 14) + sig_data(1, LOT_PORT, 3, MIME_ART) +
                sig_service(2) + sig_name(b"Caf\xe9 data") + sig_data(0, STREAM_PORT, 0, MIME_TEXT) + sig_data(1, PACKET_PORT, 1, MIME_TEXT) +
                sig_data(2, ODD_PORT, 2, MIME_TEXT) + sig_data(3, LOT_PORT_B, 3, MIME_LOGO))


def _bytes(rng, n: int) -> bytes:
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


def file_packets(rng, lot: int, size: int, name: bytes, mime: int = MIME_ART, port: int = LOT_PORT, header_at: int = 0, order=None, body: bytes | None = None):
    """-> (the packets of a whole file -- the header rides on fragment header_at --, its bytes)"""
    body = _bytes(rng, size) if body is None else body
    nfrag = (size + 255) // 256
    out = []
    for k in (order if order is not None else range(nfrag)):
        out.append((port, 100 + k, lot_packet(lot, k, body[256 * k:256 * k + 256], lot_header(size, mime, name) if k == header_at else b"", repeat=k % 3)))
    return out, body


# ---- the lists -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def files():
    """routing and the file sizes: packets in front of the SIG, the SIG, a second SIG, every port range, component types 0 / 1 / 3 / 2, PSD-port packets
    in between; files of 1, 256, 257 (out of order, repeated; the header on the last packet), 512 (its last fragment 255 bytes) and 300 bytes (the
    header behind all fragments); fragments of 0, 1, 255, 256 and 257 bytes; seq 255 and 256"""
    rng = np.random.default_rng(7001)
    p = [(LOT_PORT, 1, lot_packet(9, 0, b"early")), (STREAM_PORT, 2, b"early stream"), psd_packet(0, 3, 40),
         (SIG_PORT, 4, STANDARD_SIG), (SIG_PORT, 5, sig_service(9) + sig_data(0, 0x2000, 0, 1)),
         (0x2000, 6, b"not in the table"), (0x0100, 7, b"unknown range"), (0x6000, 8, b"unknown range"), (0x0400, 9, b""), (0x5200, 10, b"x"),
         (STREAM_PORT, 11, _bytes(rng, 301)), (PACKET_PORT, 12, _bytes(rng, 17)), (ODD_PORT, 13, b"type 2"), (STREAM_PORT, 14, b""), psd_packet(3, 15, 123)]
    sent = {}
    f1, sent[1] = file_packets(rng, 1, 1, b"one.txt", MIME_TEXT)
    f2, sent[2] = file_packets(rng, 2, 256, b"exact.png")
    f3, sent[3] = file_packets(rng, 3, 257, b"over.jpg", order=(1, 1, 0), header_at=0)
    body4 = _bytes(rng, 511) + b"\0"
    f4 = [(LOT_PORT, 40, lot_packet(4, 1, body4[256:511])), (LOT_PORT, 41, lot_packet(4, 0, body4[:256], lot_header(512, MIME_ART, b"short tail")))]
    sent[4] = body4
    body6 = _bytes(rng, 300)
    f6 = [(LOT_PORT_B, 60, lot_packet(6, 0, body6[:256])), (LOT_PORT_B, 61, lot_packet(6, 1, body6[256:])),
          (LOT_PORT_B, 62, lot_packet(6, 0, b"", lot_header(300, MIME_LOGO, b"logo.png"))), (LOT_PORT_B, 63, lot_packet(6, 1, body6[256:]))]
    sent[6] = body6
    f5 = [(LOT_PORT, 50, lot_packet(5, 0, b"", lot_header(0, MIME_ART, b"empty"))), (LOT_PORT, 51, lot_packet(5, 255, b"z")),
          (LOT_PORT, 52, lot_packet(5, 256, b"dropped")), (LOT_PORT, 53, lot_packet(5, 3, _bytes(rng, 257))), (LOT_PORT, 54, lot_packet(5, 3, _bytes(rng, 256))),
          (LOT_PORT, 55, lot_packet(5, 4, _bytes(rng, 255))), (LOT_PORT, 56, lot_packet(5, 4, _bytes(rng, 255)))]
    p += f1 + [psd_packet(0, 16, 4)] + f2 + f3 + [psd_packet(1, 17, 8)] + f4 + f5 + [psd_packet(0, 18, 2)] + f6
    return {"packets": p, "lot_files": 16, "ref": True, "sent": sent}


@functools.lru_cache(maxsize=None)
def headers():
    """hdrlen 7, 8, 15, 23, 24 (an empty name), 24 + 231 (the longest name) and hdrlen > len; a name holding a NUL, sent three times, then as it is kept"""
    rng = np.random.default_rng(7002)
    long_name = bytes(65 + k % 26 for k in range(231))
    p = [(SIG_PORT, 0, STANDARD_SIG),
         (LOT_PORT, 1, lot_packet(10, 0, b"hdrlen 7", hdrlen=7)), (LOT_PORT, 2, lot_packet(10, 0, b"hdrlen 8")),
         (LOT_PORT, 3, lot_packet(11, 0, bytes(7) + b"tail", hdrlen=15)), (LOT_PORT, 4, lot_packet(11, 0, b"stamped before")),
         (LOT_PORT, 5, lot_packet(12, 0, bytes(15) + b"tail", hdrlen=23)),
         (LOT_PORT, 6, lot_packet(13, 0, b"abc", lot_header(3, MIME_TEXT, b""))),
         (LOT_PORT, 7, lot_packet(14, 0, b"", lot_header(5, MIME_TEXT, long_name))), (LOT_PORT, 8, lot_packet(14, 0, b"12345")),
         (LOT_PORT, 9, lot_packet(15, 0, b"short", hdrlen=200)), (LOT_PORT, 10, lot_packet(15, 0, b"", hdrlen=9)),
         (LOT_PORT, 11, lot_packet(16, 0, b"nul", lot_header(3, MIME_TEXT, b"ab\0cd"))), (LOT_PORT, 12, lot_packet(16, 0, b"nul", lot_header(3, MIME_TEXT, b"ab\0cd"))),
         (LOT_PORT, 13, lot_packet(16, 0, b"nul", lot_header(3, MIME_TEXT, b"ab\0cd"))), (LOT_PORT, 14, lot_packet(16, 0, b"nul", lot_header(3, MIME_TEXT, b"ab")))]
    return {"packets": p, "lot_files": 16, "ref": True, "long_name": long_name}


CHANGES = ("size", "mime", "name", "name_len", "year", "mon", "mday", "hour", "min")


@functools.lru_cache(maxsize=None)
def changes():
    """a complete two-fragment file whose header comes again with size, mime, name and every expiry field changed in turn: each time the file starts over"""
    rng = np.random.default_rng(7003)
    body = _bytes(rng, 400)
    cur = {"size": 400, "mime": MIME_ART, "name": b"cover.jpg", "expiry": list(EXPIRY)}
    hdr = lambda: lot_header(cur["size"], cur["mime"], cur["name"], tuple(cur["expiry"]))
    p = [(SIG_PORT, 0, STANDARD_SIG), (LOT_PORT, 1, lot_packet(7, 0, body[:256], hdr())), (LOT_PORT, 2, lot_packet(7, 1, body[256:])),
         (LOT_PORT, 3, lot_packet(7, 0, body[:256], hdr()))]
    for k, what in enumerate(CHANGES):
        if what == "size":
            cur["size"] = 399
        elif what == "mime":
            cur["mime"] = MIME_LOGO
        elif what == "name":
            cur["name"] = b"cover.png"
        elif what == "name_len":
            cur["name"] = b"cover.pn"
        else:
            cur["expiry"][("year", "mon", "mday", "hour", "min").index(what)] -= 1
        p += [(LOT_PORT, 10 + 2 * k, lot_packet(7, 1, body[256:], hdr())), (LOT_PORT, 11 + 2 * k, lot_packet(7, 0, body[:256]))]
    return {"packets": p, "lot_files": 16, "ref": True}


@functools.lru_cache(maxsize=None)
def lru():
    """13 lots on one component, the first touched again in between: the 13th takes the place of the second; a file that starts over in between holds the
    counter's value, which the next packet's file gets as well -- the first of equals goes"""
    p = [(SIG_PORT, 0, STANDARD_SIG)]
    p += [(LOT_PORT, 1 + k, lot_packet(100 + k, 0, b"file %d" % k, lot_header(6 + (k > 9), MIME_ART, b"f%d" % k))) for k in range(12)]
    p += [(LOT_PORT, 20, lot_packet(100, 1, b"touch")),
          (LOT_PORT, 21, lot_packet(112, 0, b"thirteenth")),       # evicts 101
          (LOT_PORT, 22, lot_packet(101, 0, b"file 1")),           # new again (evicts 102), not a duplicate
          (LOT_PORT, 23, lot_packet(100, 0, b"file 0")),           # still there: a duplicate
          (LOT_PORT, 24, lot_packet(103, 0, b"file 3", lot_header(7, MIME_ART, b"f3"))),     # starts over: its timestamp = the counter
          (LOT_PORT, 25, lot_packet(104, 1, b"same stamp")),       # ... which this packet's file gets too
          (LOT_PORT, 26, lot_packet(105, 1, b"x")), (LOT_PORT, 27, lot_packet(106, 1, b"x")), (LOT_PORT, 28, lot_packet(107, 1, b"x")),
          (LOT_PORT, 29, lot_packet(108, 1, b"x")), (LOT_PORT, 30, lot_packet(109, 1, b"x")), (LOT_PORT, 31, lot_packet(110, 1, b"x")),
          (LOT_PORT, 32, lot_packet(111, 1, b"x")), (LOT_PORT, 33, lot_packet(112, 1, b"x")), (LOT_PORT, 34, lot_packet(101, 1, b"x")),
          (LOT_PORT, 35, lot_packet(100, 2, b"x")),
          (LOT_PORT, 36, lot_packet(120, 0, b"evicts 103, the first of the two equals")), (LOT_PORT, 37, lot_packet(104, 1, b"same stamp")),
          (LOT_PORT, 38, lot_packet(103, 0, b"file 3"))]
    return {"packets": p, "lot_files": 16, "ref": True}


@functools.lru_cache(maxsize=None)
def pool():
    """a pool of three slots under four live files of two components: the stream's least recently stamped file goes, and a counter says so"""
    p = [(SIG_PORT, 0, STANDARD_SIG),
         (LOT_PORT, 1, lot_packet(1, 0, b"a0")), (LOT_PORT_B, 2, lot_packet(1, 0, b"b0")), (LOT_PORT, 3, lot_packet(2, 0, b"a1")), (LOT_PORT, 4, lot_packet(1, 1, b"a0+")),
         (LOT_PORT_B, 5, lot_packet(2, 0, b"b1")),                  # the pool is full: b0 (lot 1 of the second component) goes
         (LOT_PORT_B, 6, lot_packet(1, 0, b"b0")),                  # new again; a1 goes
         (LOT_PORT, 7, lot_packet(1, 0, b"a0")),                    # still there
         (LOT_PORT, 8, lot_packet(2, 0, b"a1", lot_header(2, MIME_ART, b"a1")))]
    return {"packets": p, "lot_files": 3, "ref": False}


@functools.lru_cache(maxsize=None)
def big():
    """a file of 65 536 bytes (256 fragments, the 64 KB copy), sent backwards, and one that announces 65 537: never complete"""
    rng = np.random.default_rng(7005)
    f, body = file_packets(rng, 500, 65536, b"big.bin", order=tuple(range(255, -1, -1)), header_at=255)
    over = [(LOT_PORT_B, 1, lot_packet(501, 0, b"x" * 256, lot_header(65537, MIME_LOGO, b"too big"))), (LOT_PORT_B, 2, lot_packet(501, 255, b"y"))]
    return {"packets": [(SIG_PORT, 0, STANDARD_SIG)] + over[:1] + f + over[1:], "lot_files": 2, "ref": False, "sent": {500: body}}


@functools.lru_cache(maxsize=None)
def aligned():
    """files of 1000, 4099 and 300 bytes completed behind PSD-port packets of 0, 4, 8 and 2 data bytes: the copy into the event arena at every alignment"""
    rng = np.random.default_rng(7006)
    p, sent = [(SIG_PORT, 0, STANDARD_SIG)], {}
    for k, (size, pad) in enumerate(((1000, 0), (4099, 4), (300, 8), (1000, 2), (4099, 12))):
        f, sent[600 + k] = file_packets(rng, 600 + k, size, b"al%d" % k, header_at=0)
        p += f[:-1] + [psd_packet(0, 50 + k, pad)] + f[-1:]
    return {"packets": p, "lot_files": 16, "ref": True, "sent": sent}


@functools.lru_cache(maxsize=None)
def short():
    """len 7, and a file whose size announces more than 65 536 bytes"""
    p = [(SIG_PORT, 0, STANDARD_SIG), (LOT_PORT, 1, bytes([8, 0, 1, 0, 0, 0, 0])), (LOT_PORT, 2, b""),
         (LOT_PORT, 3, lot_packet(1, 0, b"ok", lot_header(2, MIME_ART, b"ok")))]
    return {"packets": p, "lot_files": 16, "ref": False}


def _with_traffic(sig: bytes, ports=(LOT_PORT, STREAM_PORT, 0x1207, 0x1210)):
    """a SIG and packets that show what the table holds afterwards"""
    return [(SIG_PORT, 0, sig)] + [(port, 1 + k, lot_packet(1, 0, b"data", lot_header(4, MIME_ART, b"n"))) for k, port in enumerate(ports)]


SIG_CASES = ("sig16", "sig9", "sigdup", "sigstray", "sigtrunc", "sigzero", "signone")


@functools.lru_cache(maxsize=None)
def sig_case(name: str):
    if name == "sig16":        # 16 services and a 17th, which ends the parse: its port is not in the table
        sig = b"".join(sig_service(200 + k, audio=k % 5 == 0) + sig_data(0, 0x1200 + k, 3 if k % 2 else 0, MIME_ART) for k in range(17)) + sig_service(1) + sig_data(0, LOT_PORT, 3, 1)
        return {"packets": _with_traffic(sig, (0x1200, 0x120F, 0x1210, LOT_PORT)), "lot_files": 4, "ref": True}
    if name == "sig9":         # 8 components and a 9th, which ends the parse: the service behind it is not in the table
        sig = sig_service(1) + sig_name(b"eight") + b"".join(sig_data(k, 0x1200 + k, 3, MIME_ART) for k in range(9)) + sig_service(2) + sig_data(0, LOT_PORT, 3, 1)
        return {"packets": _with_traffic(sig, (0x1200, 0x1207, 0x1208, LOT_PORT)), "lot_files": 4, "ref": True}
    if name == "sigdup":       # service 1 comes twice (the second clears the first: its name and LOT_PORT are gone); component 2 of service 5 comes twice
        sig = (sig_service(1) + sig_name(b"first") + sig_data(0, LOT_PORT, 3, 1) + sig_service(5) + sig_data(2, 0x1207, 0, 2) + sig_audio(3, 1, 7) +
               sig_data(2, 0x1210, 3, 3) + sig_service(1, audio=True) + sig_audio(0, 0, 9) + sig_data(1, STREAM_PORT, 0, 4))
        return {"packets": _with_traffic(sig), "lot_files": 4, "ref": True}
    if name == "sigstray":     # a stray byte ends the parse; what stood in front of it counts; an element of another 0x6x type is skipped
        sig = sig_service(1) + bytes([0x6A, 4, 1, 2, 3]) + sig_data(0, LOT_PORT, 3, 1) + b"\x00" + sig_data(1, STREAM_PORT, 0, 2)
        return {"packets": _with_traffic(sig), "lot_files": 4, "ref": True}
    if name == "sigtrunc":     # a component cut by the end of the packet
        sig = sig_service(1) + sig_data(0, LOT_PORT, 3, 1) + sig_data(1, STREAM_PORT, 0, 2)[:9]
        return {"packets": _with_traffic(sig), "lot_files": 4, "ref": False}
    if name == "sigzero":      # l == 0
        sig = sig_service(1) + sig_data(0, LOT_PORT, 3, 1) + bytes([0x67, 0]) + sig_data(1, STREAM_PORT, 0, 2)
        return {"packets": _with_traffic(sig), "lot_files": 4, "ref": False}
    if name == "signone":      # no service (a component in front of any; then a stray byte at once): an event with an empty table each time, and the next SIG is parsed
        p = [(SIG_PORT, 0, sig_data(0, LOT_PORT, 3, 1) + sig_service(1)), (LOT_PORT, 1, lot_packet(1, 0, b"dropped")), (SIG_PORT, 2, b"\x12" + sig_service(1)),
             (SIG_PORT, 3, b"")] + _with_traffic(STANDARD_SIG)
        return {"packets": p, "lot_files": 4, "ref": False}
    raise KeyError(name)


_BY_NAME = {"files": files, "headers": headers, "changes": changes, "lru": lru, "pool": pool, "big": big, "aligned": aligned, "short": short,
            **{n: functools.partial(sig_case, n) for n in SIG_CASES}}
NAMES = tuple(_BY_NAME)


def get(name: str):
    return _BY_NAME[name]()


@functools.lru_cache(maxsize=None)
def carousel(rounds: int = 1):
    """what a station repeats: the SIG, two small files and ID3 packets, `rounds` times over"""
    rng = np.random.default_rng(7010)
    f1, b1 = file_packets(rng, 700, 700, b"cover.jpg", header_at=0)
    f2, b2 = file_packets(rng, 701, 300, b"logo.png", MIME_LOGO, LOT_PORT_B, header_at=0)
    one = [(SIG_PORT, 0, STANDARD_SIG), psd_packet(0, 1, 60)] + f1 + [psd_packet(1, 2, 45)] + f2
    return {"packets": one * rounds, "lot_files": 4, "ref": True, "sent": {700: b1, 701: b2}, "one": one}


def psd_frames(packets, per_frame: int = 10, span: int = 236):
    """a packet list as a PSD byte stream of program 0 (synth_l2.hdlc / aas_payload), cut into spans of `span` bytes, per_frame PDUs per P1 frame, with the
    builders tests/psd_args.py uses -> [nframes, 146176] bits"""
    from tests import psd_args as pa
    rng = np.random.default_rng(7011)
    stream = b"\x7e" + b"".join(pa.hdlc(pa.aas_payload(pk[0], pk[1], pk[2])) for pk in packets)
    total = per_frame * span
    stream += b"\x7e" * (-len(stream) % total)
    frames = []
    for fi in range(len(stream) // total):
        body = b""
        for q in range(per_frame):
            at = fi * total + q * span
            body += pa._pdu(rng, 1500, 0, 0, stream[at:at + span], nop=2, seq=(fi * per_frame + q) % 64, pdu_seq=fi % 8)
        frames.append(synth_l2.frame_from_bytes(body, 146176))
    return np.stack(frames)
