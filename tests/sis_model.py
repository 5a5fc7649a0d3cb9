"""The rules of pids_frame_push / sis_decode (pids.c:935-1050) restated in Python, frame by frame: what csrc/k_sis.hip is compared with
(tests/sis_checks.py), and itself pinned to the UNMODIFIED reference (tests/test_sis_stage_cpu.py: RefSis below drives the reference through its
public API and, for frame sets without a capture, through its own pids_frame_push).  An event is (kind, v, enc, data) as the device delivers it:
kind a name of eng.SIS_KINDS, v eight int32, data the raw text bytes."""
from __future__ import annotations

import ctypes

import numpy as np

from nrsc5_amd import engine as eng, synth

STATS = eng.SIS_STATS[:-1]
CHARS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ ?-*$ "
SIZES = (32, 22, 58, 32, 27, 58, 27, 22, 58, 58, 27, -1, -1, -1, -1, -1)


def _int(bits, off, n):
    v = 0
    for k in range(n):
        v = (v << 1) | int(bits[off + k])
    return v


def _bytes(bits, off, n):
    return bytes(_int(bits, off + 8 * k, 8) for k in range(n))


def _cstr(buf) -> bytes:
    return bytes(buf).split(b"\0", 1)[0]


class SisModel:
    def __init__(self):
        self.stats = dict.fromkeys(STATS, 0)
        self.reset()

    def reset(self):                                            # pids_init
        self.cc, self.fcc, self.short_name = b"", -1, b""
        self.long_name, self.long_have, self.long_seq, self.long_displayed = bytearray(57), [0] * 8, -1, 0
        self.lat = self.lon = None
        self.altitude = 0
        self.message, self.msg_have, self.msg_seq, self.msg_displayed = bytearray(191), [0] * 32, -1, 0
        self.msg_priority = self.msg_enc = self.msg_len = self.msg_checksum = 0
        self.asd = [(-1, -1, -1)] * 8
        self.dsd = [(-1, -1, -1)] * 16
        self.params = [-1] * 13
        self.usn, self.usn_final, self.usn_have = bytearray(13), b"", [0, 0]
        self.usn_enc, self.usn_append, self.usn_len, self.usn_displayed = 0, -1, -1, 0
        self.slogan, self.slogan_have, self.slogan_enc, self.slogan_len, self.slogan_displayed = bytearray(96), [0] * 16, 0, -1, 0
        self._reset_alert()
        # (pids_init leaves alert_len as it is -- zero in a fresh session -- and tests `alert_len >= 0`; no value it can hold completes an alert
        # before frame 0 has set it again, so zero stands for all of them)
        self.alert_enc = self.alert_len = self.alert_crc = self.alert_cnt_len = 0

    def _reset_alert(self):
        self.alert, self.alert_have, self.alert_seq, self.alert_displayed, self.alert_timeout = bytearray(382), [0] * 64, -1, 0, 0

    # ---- pids_frame_push ----
    def push(self, frame) -> list:
        """one frame as handed to pids_frame_push -> its events, in callback order"""
        self.ev = []
        bits = synth._rev8(np.asarray(frame, dtype=np.uint8))
        self.stats["frames"] += 1
        if _int(bits, 68, 12) != synth.crc12(bits):
            return []
        self.stats["crc_good"] += 1
        if bits[0]:
            self.stats["llds"] += 1
            return []
        self.stats["sis"] += 1
        b = bits[1:]
        if self.alert_displayed:
            self.alert_timeout += 1
        off = 1
        for _ in range(int(b[0]) + 1):
            if off > 59:
                break
            mid = _int(b, off, 4)
            off += 4
            size = SIZES[mid]
            if size == -1:
                self.stats["unknown_id"] += 1
                break
            if off > 63 - size:
                self.stats["no_room"] += 1
                break
            self.stats["id%d" % mid] += 1
            handler = getattr(self, "_id%d" % mid, None)
            if handler is not None:
                handler(b[off:off + size])
            off += size
        if self.alert_displayed and self.alert_timeout >= 16:
            self._reset_alert()
            self._emit("alert", [-1])
        return self.ev

    def _emit(self, kind, v=(), enc=0, data=b""):
        self.stats["events"] += 1
        self.ev.append((kind, list(v) + [0] * (8 - len(v)), enc, bytes(data)))

    def _id0(self, p):
        cc, fcc = (CHARS[_int(p, 0, 5)] + CHARS[_int(p, 5, 5)]).encode(), _int(p, 13, 19)
        if cc != self.cc or fcc != self.fcc:
            self.cc, self.fcc = cc, fcc
            self._emit("station_id", [fcc], 0, cc)

    def _id1(self, p):
        name = "".join(CHARS[_int(p, 5 * k, 5)] for k in range(4)).encode() + (b"-FM" if (p[20], p[21]) == (0, 1) else b"")
        if name != self.short_name:
            self.short_name = name
            self._emit("station_name", [], 0, name)

    def _id2(self, p):
        last, cur, seq = _int(p, 0, 3), _int(p, 3, 3), _int(p, 55, 3)
        if cur == 0 and seq != self.long_seq:
            self.long_name, self.long_have, self.long_seq, self.long_displayed = bytearray(57), [0] * 8, seq, 0
        self.long_name[7 * cur:7 * cur + 7] = bytes(_int(p, 6 + 7 * k, 7) for k in range(7))
        self.long_have[cur] = 1
        if self.long_seq >= 0 and not self.long_displayed and all(self.long_have[:last + 1]):
            self.long_displayed = 1
            if not self.slogan_displayed:
                self._emit("station_slogan", [], 0, _cstr(self.long_name))

    def _id4(self, p):
        v = _int(p, 1, 22)
        v = v - (1 << 22) if v & (1 << 21) else v
        if p[0]:
            high = _int(p, 23, 4) << 8
            if v != self.lat or high != (self.altitude & 0xf00):
                self.lat, self.altitude = v, (self.altitude & 0x0f0) | high
                if self.lon is not None:
                    self._emit("station_location", [self.lat, self.lon, self.altitude])
        else:
            low = _int(p, 23, 4) << 4
            if v != self.lon or low != (self.altitude & 0x0f0):
                self.lon, self.altitude = v, (self.altitude & 0xf00) | low
                if self.lat is not None:
                    self._emit("station_location", [self.lat, self.lon, self.altitude])

    def _id5(self, p):
        cur, seq = _int(p, 0, 5), _int(p, 5, 2)
        if cur == 0:
            if seq != self.msg_seq:
                self.message, self.msg_have, self.msg_seq, self.msg_displayed = bytearray(191), [0] * 32, seq, 0
            self.msg_priority, self.msg_enc, self.msg_len, self.msg_checksum = int(p[7]), _int(p, 8, 3), _int(p, 11, 8), _int(p, 19, 7)
            self.message[0:4] = _bytes(p, 26, 4)
        else:
            self.message[6 * cur - 2:6 * cur + 4] = _bytes(p, 10, 6)
        self.msg_have[cur] = 1
        if self.msg_seq >= 0 and not self.msg_displayed:
            need = (self.msg_len + 7) // 6
            if need > 32:                                       # the reference reads past message_have_frame here: never complete
                self.stats["never_complete_message"] += 1
                return
            if all(self.msg_have[:need]):
                s = sum(self.message[:self.msg_len])
                if ((((s >> 8) & 0x7f) + (s & 0xff)) & 0x7f) == self.msg_checksum:
                    self.msg_displayed = 1
                    self._emit("station_message", [self.msg_priority], self.msg_enc, self.message[:self.msg_len])
                else:
                    self.stats["bad_checksum"] += 1

    def _id6(self, p):
        cat = _int(p, 0, 2)
        if cat == 0:
            prog, new = _int(p, 3, 6), (int(p[2]), _int(p, 9, 8), _int(p, 22, 5))
            if prog < 8 and self.asd[prog] != new:
                self.asd[prog] = new
                self._emit("audio_service", [prog, *new])
        elif cat == 1:
            new = (int(p[2]), _int(p, 3, 9), _int(p, 15, 12))
            for k in range(16):
                if self.dsd[k] == new:
                    break
                if self.dsd[k][1] == -1:
                    self.dsd[k] = new
                    self._emit("data_service", list(new))
                    break

    _id10 = _id6

    def _id7(self, p):
        index, value = _int(p, 0, 6), _int(p, 6, 16)
        if index >= 13 or self.params[index] == value:
            return
        self.params[index] = value
        q = self.params
        if index <= 2:
            if min(q[0:3]) >= 0:
                alfn = (q[2] << 16 | q[1]) & 0xffffffff
                self._emit("leap_second", [q[0] >> 8, q[0] & 0xff, alfn - (1 << 32) if alfn & (1 << 31) else alfn])
        elif index == 3:
            tzo = (q[3] >> 5) & 0x7ff
            self._emit("local_time", [tzo - 2048 if tzo >= 1024 else tzo, q[3] & 1, (q[3] >> 1) & 1, (q[3] >> 2) & 7])
        elif index <= 7:
            if min(q[4:8]) >= 0:
                self._emit("exciter", q[4:8])
        elif index <= 11:
            if min(q[8:12]) >= 0:
                self._emit("importer", q[8:12])

    def _id8(self, p):
        cur = _int(p, 0, 4)
        if p[4] == 0:
            if cur >= 2:
                return
            if cur == 0:
                self.usn_enc, self.usn_append, self.usn_len = _int(p, 5, 3), int(p[8]), int(p[9]) + 1
            self.usn[6 * cur:6 * cur + 6] = _bytes(p, 10, 6)
            self.usn_have[cur] = 1
            if self.usn_len >= 0 and not self.usn_displayed and all(self.usn_have[:self.usn_len]):
                self.usn_final = _cstr(self.usn) + (b"-FM" if self.usn_append else b"")
                self.usn_displayed = 1
                self._emit("station_name", [], self.usn_enc, self.usn_final)
        else:
            if cur == 0:
                self.slogan_enc, self.slogan_len = _int(p, 5, 3), _int(p, 11, 7)
                self.slogan[0:5] = _bytes(p, 18, 5)
            else:
                self.slogan[6 * cur - 1:6 * cur + 5] = _bytes(p, 10, 6)
            self.slogan_have[cur] = 1
            if self.slogan_len >= 0 and not self.slogan_displayed:
                need = (self.slogan_len + 6) // 6
                if need > 16:                                   # past slogan_have_frame: never complete
                    self.stats["never_complete_slogan"] += 1
                    return
                if all(self.slogan_have[:need]):
                    self.slogan_displayed = 1
                    if not self.long_displayed:
                        self._emit("station_slogan", [], self.slogan_enc, self.slogan[:self.slogan_len])

    def _id9(self, p):
        cur, seq = _int(p, 0, 6), _int(p, 6, 2)
        self.alert_timeout = 0
        if cur == 0:
            if seq != self.alert_seq:
                self.alert, self.alert_have, self.alert_seq, self.alert_displayed = bytearray(382), [0] * 64, seq, 0
            self.alert_enc, self.alert_len, self.alert_crc, self.alert_cnt_len = _int(p, 10, 3), _int(p, 13, 9), _int(p, 22, 7), 1 + 2 * _int(p, 29, 5)
            self.alert[0:3] = _bytes(p, 34, 3)
        else:
            self.alert[6 * cur - 3:6 * cur + 3] = _bytes(p, 10, 6)
        self.alert_have[cur] = 1
        if self.alert_len >= 0 and not self.alert_displayed:
            need = (self.alert_len + 8) // 6
            if need > 64:                                       # past alert_have_frame: never complete
                self.stats["never_complete_alert"] += 1
                return
            if not all(self.alert_have[:need]):
                return
            if self.alert_crc != synth.sis_crc7(bytes(self.alert[:self.alert_len])):
                self.stats["bad_crc7"] += 1
            elif self.alert_cnt_len < 7 or self.alert_len < self.alert_cnt_len:
                self.stats["bad_cnt_len"] += 1
            elif ((self.alert[2] & 0x0f) << 8 | self.alert[1]) != synth.sis_cnt_crc(bytes(self.alert[:self.alert_cnt_len])):
                self.stats["bad_cnt_crc"] += 1
            else:
                self.alert_displayed = 1
                self._emit("alert", [self.alert_cnt_len], self.alert_enc, self.alert[:self.alert_len])

    # ---- report(), pids.c:284-383 ----
    def info(self) -> dict:
        """(a frame 0 with the same seq rewrites the length of a displayed item unchecked; the snapshot shows at most what the buffers hold)"""
        f32 = lambda i: float(np.float32(i) / np.float32(8192))
        slogan_len, msg_len, alert_len = min(self.slogan_len, 95), min(self.msg_len, 190), min(self.alert_len, 381)
        cnt_len = min(self.alert_cnt_len, alert_len)
        if self.usn_displayed:
            name = eng.sis_text(self.usn_enc, self.usn_final)
        else:
            name = self.short_name.decode() if self.short_name else None
        if self.slogan_displayed:
            slogan = eng.sis_text(self.slogan_enc, bytes(self.slogan[:slogan_len]))
        else:
            slogan = eng.sis_text(0, _cstr(self.long_name)) if self.long_displayed else None
        return {"country": self.cc.decode() or None, "fcc": self.fcc, "name": name, "slogan": slogan,
                "message": eng.sis_text(self.msg_enc, bytes(self.message[:msg_len])) if self.msg_displayed else None,
                "alert": eng.sis_text(self.alert_enc, bytes(self.alert[cnt_len:alert_len])) if self.alert_displayed else None,
                "alert_control_data": bytes(self.alert[:cnt_len]) if self.alert_displayed else None,
                "location": None if self.lat is None or self.lon is None else (f32(self.lat), f32(self.lon), self.altitude),
                "audio_services": [(k, *a) for k, a in enumerate(self.asd) if a[1] != -1], "data_services": [d for d in self.dsd if d[1] != -1]}


def run(frames, reset_at=None, model: SisModel | None = None):
    """-> (per frame [event], the model): the model over frames; reset_at: the state is reset in front of that frame (== len(frames): behind the last)"""
    m = model or SisModel()
    per = []
    for k, f in enumerate(frames):
        if k == reset_at:
            m.reset()
        per.append(m.push(f))
    if reset_at is not None and reset_at == len(frames):
        m.reset()
    return per, m


def fields(ev) -> tuple:
    """(kind, fields) as SisConsumer.events holds them"""
    kind, v, enc, data = ev
    return kind, eng.sis_event_fields(kind, v, enc, data)


def ref_form(ev) -> tuple:
    """an event in the form RefSis records the reference's callbacks in: text as the UTF-8 bytes of the C string (None: a NULL string)"""
    kind, v, enc, data = ev
    if kind == "station_id":
        return kind, data, v[0]
    if kind in ("station_name", "station_slogan", "station_message"):
        return kind, eng.sis_utf8(enc, data)
    if kind == "station_location":
        return kind, float(np.float32(v[0]) / np.float32(8192)), float(np.float32(v[1]) / np.float32(8192)), v[2]
    if kind == "audio_service":
        return (kind, *v[:4])
    if kind == "data_service":
        return (kind, *v[:3])
    if kind == "alert":
        return (kind, None, None) if v[0] < 0 else (kind, eng.sis_utf8(enc, data[v[0]:]), data[:v[0]])
    if kind == "leap_second":
        return kind, v[0], v[1], v[2] & 0xffffffff
    if kind == "local_time":
        return (kind, *v[:4])
    d = eng.sis_event_fields(kind, v, enc, data)
    out = (kind, d["manufacturer_id"].encode("latin-1"), tuple(d["core_version"]), d["core_status"], tuple(d["manufacturer_version"]), d["manufacturer_status"])
    return out + ((d["importer_connected"],) if kind == "exciter" else ())


# ---- the unmodified reference: its public API (include/nrsc5.h) through ctypes ------------------------------------------------------------------
class _Station(ctypes.Structure):
    _fields_ = [("country_code", ctypes.c_char_p), ("fcc_facility_id", ctypes.c_int)]


class _Text(ctypes.Structure):
    _fields_ = [("text", ctypes.c_char_p)]


class _Location(ctypes.Structure):
    _fields_ = [("latitude", ctypes.c_float), ("longitude", ctypes.c_float), ("altitude", ctypes.c_int)]


class _Asd(ctypes.Structure):
    _fields_ = [("program", ctypes.c_uint), ("access", ctypes.c_uint), ("type", ctypes.c_uint), ("sound_exp", ctypes.c_uint)]


class _Dsd(ctypes.Structure):
    _fields_ = [("access", ctypes.c_uint), ("type", ctypes.c_uint), ("mime_type", ctypes.c_uint32)]


class _Alert(ctypes.Structure):
    _fields_ = [("message", ctypes.c_char_p), ("control_data", ctypes.POINTER(ctypes.c_uint8)), ("control_data_length", ctypes.c_int),
                ("category1", ctypes.c_int), ("category2", ctypes.c_int), ("location_format", ctypes.c_int), ("num_locations", ctypes.c_int),
                ("locations", ctypes.POINTER(ctypes.c_int))]


class _Exciter(ctypes.Structure):
    _fields_ = [("manufacturer_id", ctypes.c_char_p), ("core_version", ctypes.c_int * 4), ("core_status", ctypes.c_int),
                ("manufacturer_version", ctypes.c_int * 4), ("manufacturer_status", ctypes.c_int), ("importer_connected", ctypes.c_int)]


class _Importer(ctypes.Structure):
    _fields_ = _Exciter._fields_[:-1]


class _Leap(ctypes.Structure):
    _fields_ = [("pending_offset", ctypes.c_int), ("current_offset", ctypes.c_int), ("pending_alfn", ctypes.c_uint)]


class _LocalTime(ctypes.Structure):
    _fields_ = [("utc_offset", ctypes.c_int), ("dst_regional", ctypes.c_int), ("dst_local", ctypes.c_int), ("dst_schedule", ctypes.c_int)]


class _Union(ctypes.Union):
    _fields_ = [("station_id", _Station), ("text", _Text), ("location", _Location), ("asd", _Asd), ("dsd", _Dsd), ("alert", _Alert),
                ("exciter", _Exciter), ("importer", _Importer), ("leap", _Leap), ("local_time", _LocalTime)]


class _Event(ctypes.Structure):                                  # struct nrsc5_event_t, include/nrsc5.h:404-613
    _anonymous_ = ("u",)
    _fields_ = [("event", ctypes.c_uint), ("u", _Union)]


_CALLBACK = ctypes.CFUNCTYPE(None, ctypes.POINTER(_Event), ctypes.c_void_p)
# NRSC5_EVENT_*, include/nrsc5.h:162-195
_EV = {15: "station_id", 16: "station_name", 17: "station_slogan", 18: "station_message", 19: "station_location", 20: "audio_service", 21: "data_service",
       22: "alert", 27: "exciter", 28: "importer", 29: "leap_second", 30: "local_time"}


class RefSis:
    """One session of the unmodified reference (oracle/_ref/libnrsc5_ref.so): nrsc5_open_pipe / nrsc5_set_callback, a ctypes callback that records the
    SIS events in ref_form's shape.  run_iq feeds samples through nrsc5_pipe_samples_cs16 / _cu8; push_frames hands frames to the reference's own
    pids_frame_push on a pids_t of the test's, whose `input` points at a stand-in that holds the session (input_t starts with the nrsc5_t pointer,
    input.h:20-22, and nrsc5_report_* reads nothing else of it)."""

    def __init__(self, reflib, mode: int = 0):
        self.lib = L = reflib.lib
        L.refh_open(mode, 0, 0)                                  # no taps from an earlier session of the harness
        L.refh_close()
        L.nrsc5_open_pipe.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        L.nrsc5_set_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.nrsc5_set_callback.argtypes = [ctypes.c_void_p, _CALLBACK, ctypes.c_void_p]
        L.nrsc5_pipe_samples_cs16.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
        L.nrsc5_pipe_samples_cu8.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
        L.nrsc5_close.argtypes = [ctypes.c_void_p]
        L.nrsc5_close.restype = None
        L.pids_init.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.pids_init.restype = None
        L.pids_frame_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.pids_frame_push.restype = None
        self.radio = ctypes.c_void_p()
        if L.nrsc5_open_pipe(ctypes.byref(self.radio)) != 0:
            raise RuntimeError("nrsc5_open_pipe failed")
        L.nrsc5_set_mode(self.radio, mode)
        self.events = []
        self._cb = _CALLBACK(self._on_event)
        L.nrsc5_set_callback(self.radio, self._cb, None)

    def _on_event(self, evt, opaque):
        e = evt.contents
        kind = _EV.get(e.event)
        if kind is None:
            return
        if kind == "station_id":
            r = (kind, e.station_id.country_code, e.station_id.fcc_facility_id)
        elif kind in ("station_name", "station_slogan", "station_message"):
            r = (kind, e.text.text)
        elif kind == "station_location":
            r = (kind, float(e.location.latitude), float(e.location.longitude), e.location.altitude)
        elif kind == "audio_service":
            r = (kind, e.asd.program, e.asd.access, e.asd.type, e.asd.sound_exp)
        elif kind == "data_service":
            r = (kind, e.dsd.access, e.dsd.type, e.dsd.mime_type)
        elif kind == "alert":
            n = e.alert.control_data_length
            r = (kind, None, None) if n < 0 else (kind, e.alert.message, bytes(e.alert.control_data[:n]))
        elif kind == "leap_second":
            r = (kind, e.leap.pending_offset, e.leap.current_offset, e.leap.pending_alfn)
        elif kind == "local_time":
            r = (kind, e.local_time.utc_offset, e.local_time.dst_regional, e.local_time.dst_local, e.local_time.dst_schedule)
        else:
            x = e.exciter if kind == "exciter" else e.importer
            r = (kind, x.manufacturer_id, tuple(x.core_version), x.core_status, tuple(x.manufacturer_version), x.manufacturer_status)
            if kind == "exciter":
                r += (x.importer_connected,)
        self.events.append(r)

    def run_iq(self, iq, chunk: int = 32768) -> list:
        iq = np.ascontiguousarray(iq)
        push = self.lib.nrsc5_pipe_samples_cu8 if iq.dtype == np.uint8 else self.lib.nrsc5_pipe_samples_cs16
        for off in range(0, iq.size, chunk):
            part = iq[off:off + chunk]
            push(self.radio, part.ctypes.data, part.size)
        return self.events

    def push_frames(self, frames) -> list:
        """-> per frame, the events the reference's pids_frame_push fired"""
        stand_in = (ctypes.c_void_p * 512)()
        stand_in[0] = self.radio.value
        st = ctypes.create_string_buffer(8192)                   # a pids_t (about 1.3 KB)
        self.lib.pids_init(st, stand_in)
        per = []
        for f in frames:
            first = len(self.events)
            b = np.ascontiguousarray(f, dtype=np.uint8)
            self.lib.pids_frame_push(st, b.ctypes.data)
            per.append(self.events[first:])
        return per

    def close(self):
        if self.radio:
            self.lib.nrsc5_close(self.radio)
            self.radio = ctypes.c_void_p()
