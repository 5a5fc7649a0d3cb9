"""Seeded PIDS frame sets for the SIS tests (tests/sis_checks.py): each is a [n, 80] uint8 array of frames as handed to pids_frame_push.
  schedule(variant)   a station's transmission built with the frame builders of nrsc5_amd/synth.py: every message id, both payload counts, and the cases
                      test_sis_stage_cpu.py asserts; never_complete=False leaves out the three lengths the reference cannot handle (what a capture for the reference carries)
  random_frames(seed) 256 frames of random payload bits with a valid CRC-12
  am_frames()         the schedule carried in an MA1 capture, as the oracle's AM receiver decodes it
  longest()           the longest message, slogan and alert that frames can carry (190, 95 and 381 bytes: every have_frame entry in use), one byte short of
                      the never-complete lengths
  relength()          ... and then a frame 0 with the same seq for each of them that rewrites the length to 255 / 127 / 511 while the item stays displayed
test_sis_stage_cpu.py asserts, on the model's and the reference's output alone, that the sets hold what they are named for."""
from __future__ import annotations

import functools

import numpy as np

from nrsc5_amd import synth as S

RANDOM_SEEDS = (1, 2, 3, 4)
NAMES = ("schedule", "schedule1", "schedule2") + tuple("random%d" % s for s in RANDOM_SEEDS) + ("am", "longest", "relength")
STATIONS = (("WXYZ", "US", 12345, b"KEXAMPLE-HD1", b"The best mix of everything"),
            ("KABC", "CA", 54321, b"Radio Nord", b"Des nouvelles du nord"),
            ("WQQQ", "US", 777, b"Q-ROCK", b"Rock around the clock, all day"))
LEAD_IN = 2


@functools.lru_cache(maxsize=None)
def schedule(variant: int = 0, never_complete: bool = True) -> np.ndarray:
    short, country, fcc, usn, slogan = STATIONS[variant]
    long_a, long_b = b"%s long nm A" % short.encode(), b"%s long B" % short.encode()        # 2 frames each (8 .. 14 characters)
    frames = []
    add = lambda *p, **kw: frames.append(S.sis_frame(list(p), **kw))
    sid, sn = S.sis_station_id(country, fcc), S.sis_short_name(short, True)
    for _ in range(LEAD_IN):                                    # what a receiver may miss while it acquires: repeated below
        add(sid, sn)
    add(sid, sn)
    add(S.sis_station_id("MX", 4242))                           # one payload; the id changes and changes back
    add(sid, (3, [1, 0] * 16))                                  # a reserved id 3 behind a payload
    add((3, [0, 1] * 16), S.sis_parameter(12, 77 + variant))    # ... and in front of one
    add((11, [1] * 20))                                         # ids without a size end the walk
    add((13 + variant % 3, [0] * 8), sn)
    msg = S.sis_message(b"Hello, %s!" % short.encode(), seq=0)
    add(S.sis_short_name(short, False), msg[0])                 # 22 + 58 bits: no room for the second payload; the name loses its -FM
    add(sn, count=1)
    add(sid, llds=True)                                         # an LLDS frame is not decoded
    add(S.sis_station_id("ZZ", 1), llds=True)
    if never_complete:                                          # lengths past the reference's have_frame arrays (no set of frames carries them)
        add(S.sis_message(b"x" * 4, seq=3, length=200)[0])
        add(S.sis_slogan(b"y" * 5, length=100)[0])
        add(S.sis_alert(S.sis_alert_control(bytes(7)), b"", seq=3, length=400)[0])
    # long name and slogan.  variant 0: the long name is reported, its next version is open when the slogan completes (reported), and then completes unseen;
    # other variants: the slogan completes while the long name is displayed (not reported)
    ln = S.sis_long_name(long_a, seq=1)
    add(ln[1]); add(ln[0]); add(ln[1])                          # out of order and repeated: frame 1 before frame 0 is cleared by frame 0's new seq
    lb = S.sis_long_name(long_b, seq=2)
    sl = S.sis_slogan(slogan)
    if variant == 0:
        add(lb[0])
    for k in [1, 0, 0] + list(range(1, len(sl))):             # out of order, frame 0 twice
        add(sl[k])
    for p in (lb[1:] if variant == 0 else lb):
        add(p)
    # universal short name in two frames, -FM appended
    un = S.sis_universal_name(usn, append=variant != 1)
    for p in reversed(un):
        add(p)
    # station message: out of order with repeats; a seq change in the middle of an item; a wrong checksum and its correction; UCS-2
    m = S.sis_message(b"Now playing on " + short.encode(), seq=1, priority=1)
    for k in (0, 2, 2, 3, 1, 1):                                # (frames in front of a frame 0 with a new seq are cleared by it)
        add(m[k % len(m)])
    m2 = S.sis_message(b"A newer message from " + short.encode(), seq=2)
    add(m2[0]); add(m2[1])
    m3 = S.sis_message(b"Traffic on I-%d" % (10 + variant), seq=3)
    for p in m3:
        add(p)
    text = b"Weather: sunny %d" % variant
    bad = S.sis_message(text, seq=0, checksum=(S.sis_message_checksum(text) + 1) & 0x7f)
    for p in (bad[0], bad[2], bad[1]):
        add(p)
    add(S.sis_message(text, seq=0)[0])                          # the correction: frame 0 again, same seq
    u = "﻿Café №%d" % variant
    for p in S.sis_message(u.encode("utf-16-le"), seq=1, enc=4):
        add(p)
    # location: longitude first
    lat, lon = int(40.5 * 8192) + variant, int(-74.25 * 8192) - variant
    loc = S.sis_location(lat, lon, 0x3a0)
    add(loc[1]); add(loc[0])
    add(S.sis_location(lat, lon, 0x4b0)[0], S.sis_location(lat, lon, 0x4b0)[1])
    # a valid alert; the frames behind it carry no alert, so it times out 16 frames later
    cnt = S.sis_alert_control(bytes([0x11, 0, 0x20, 0x33, 0x44 + variant, 0x55, 0x66]))
    al = S.sis_alert(cnt, b"Tornado!%d" % variant, seq=1)
    for k in (1, 0, 2, 1, 3):
        add(al[k % len(al)])
    # service descriptors: 9 audio services (one with a program number >= 8), 17 distinct data services (16 slots)
    aud = [S.sis_audio_service(p, p & 1, 10 + p + variant, p % 3, msg_id=6 if p % 2 else 10) for p in range(8)] + [S.sis_audio_service(9, 0, 1, 2)]
    dat = [S.sis_data_service(k & 1, 256 + k, 0x100 + 17 * k + variant, msg_id=10 if k % 3 == 0 else 6) for k in range(17)]
    both = aud + dat
    for k in range(0, len(both), 2):
        add(*both[k:k + 2])
    add(dat[3], aud[2])                                         # known ones again: nothing to report
    # the 13 parameters, their groups completing in scrambled order; an index the table lacks; a change
    par = {0: 0x1213, 1: 0x0100, 2: 0x0002, 3: (0x7c4 << 5) | 0b01101, 4: (ord("G") << 8) | 0x80 | ord("G"), 5: 0x0a53, 6: 0x1863, 7: 0x2b5a,
           8: (ord("L") << 8) | ord("7"), 9: 0x0842, 10: 0x10c6, 11: 0x1ae9, 12: 5}
    order = (2, 5, 0, 9, 1, 7, 4, 3, 11, 6, 8, 20, 10, 12, 1)
    ps = [S.sis_parameter(i, (par[i] + variant) & 0xffff if i in par else 1) for i in order]
    ps[-1] = S.sis_parameter(1, 0x0200)
    for k in range(0, len(ps) - 1, 2):
        add(*ps[k:k + 2])
    add(ps[-1])
    # alerts that must not show: a bad crc7, a bad control-data CRC, a control-data length below 7
    a1 = S.sis_alert(cnt, b"x1", seq=2, crc7=(S.sis_crc7(cnt + b"x1") ^ 1))
    broken = bytearray(cnt); broken[1] ^= 0x40
    a2 = S.sis_alert(bytes(broken), b"x2", seq=3)
    a3 = S.sis_alert(S.sis_alert_control(bytes([1, 0, 0, 3, 4])), b"x3y", seq=0)
    for a in (a1, a2, a3):
        for p in a:
            add(p)
    add(sid, sn)
    out = []
    for k, f in enumerate(frames):                              # about every 7th frame arrives with a broken CRC: a station id that must not show
        out.append(f)
        if k % 6 == 5:
            out.append(S.sis_frame([S.sis_station_id("QQ", 99)], corrupt=True))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def random_frames(seed: int, n: int = 256) -> np.ndarray:
    rng = np.random.default_rng(1000 + seed)
    out = []
    for _ in range(n):
        logical = np.zeros(80, dtype=np.uint8)
        logical[0] = rng.integers(0, 8) == 0                    # one frame in eight is LLDS
        logical[1:68] = rng.integers(0, 2, size=67)
        c = S.crc12(logical)
        logical[68:80] = [(c >> (11 - k)) & 1 for k in range(12)]
        out.append(S._rev8(logical))
    return np.stack(out)


AM_FRAMES = 16                                                  # L1 frames of the MA1 capture: 8 PIDS frames each


@functools.lru_cache(maxsize=None)
def am_capture():
    from nrsc5_amd import synth_am
    return synth_am.am_ma1_capture(AM_FRAMES, seed=11, cfo_hz=2.0, offset=600, pids=schedule(0, never_complete=False))


@functools.lru_cache(maxsize=None)
def am_frames() -> np.ndarray:
    from oracle import port
    log, _, _ = port.Oracle().run(am_capture().iq, mode=1)
    return np.stack([v["bits"] for k, v in log if k == "pids"])


LONGEST = (190, 95, 381)


@functools.lru_cache(maxsize=None)
def longest() -> np.ndarray:
    rng = np.random.default_rng(7)
    text = lambda n: bytes(rng.integers(0x20, 0x7f, size=n, dtype=np.uint8))
    cnt = S.sis_alert_control(bytes(rng.integers(0, 256, size=63, dtype=np.uint8)))       # the longest control data: 63 bytes
    items = [S.sis_message(text(LONGEST[0]), seq=1), S.sis_slogan(text(LONGEST[1])), S.sis_alert(cnt, text(LONGEST[2] - 63), seq=2)]
    assert [len(i) for i in items] == [32, 16, 64]
    return np.stack([S.sis_frame([p]) for item in items for p in reversed(item[1:] + item[:1])])    # (frame 0 first, then the others from the last down)


RELENGTH = (255, 127, 511)


@functools.lru_cache(maxsize=None)
def relength() -> np.ndarray:
    """the longest items displayed, a location and two services known, and then a frame 0 with the same seq for each item that rewrites its length to the
    largest the field holds (255, 127, 511; control data 63): nothing checks a length while its item stays displayed, and the snapshot must not follow it
    past the buffers"""
    loc = S.sis_location(int(12.5 * 8192), int(-3.25 * 8192), 0x120)
    tail = [[loc[0], loc[1]], [S.sis_audio_service(1, 0, 5, 2), S.sis_data_service(1, 300, 0x123)],
            [S.sis_message(b"MSG!", seq=1, length=RELENGTH[0])[0]], [S.sis_slogan(b"SLOGN", length=RELENGTH[1])[0]],
            [S.sis_alert(b"\x01\x02\x03", b"", seq=2, length=RELENGTH[2], cnt_len=63)[0]], [S.sis_parameter(3, 0x1234)]]
    return np.concatenate([longest(), np.stack([S.sis_frame(g) for g in tail])])


def frames(name: str) -> np.ndarray:
    if name == "relength":
        return relength()
    if name == "am":
        return am_frames()
    if name == "longest":
        return longest()
    if name.startswith("random"):
        return random_frames(int(name[6:]))
    return schedule(int(name[8:] or 0))
