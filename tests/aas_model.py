"""The rules of output_aas_push / parse_sig / process_port (output.c:493-896) restated in Python, packet by packet, with the deviations include/nrsc5hip.h
states: what csrc/k_aas.hip is compared with (tests/aas_checks.py), and itself pinned to the UNMODIFIED reference (RefAas below hands packets to the
reference's own output_aas_push).  An event is (kind, port, seq, v, data) as the device delivers it: kind a name of eng.AAS_KINDS, v eight int32."""
from __future__ import annotations

import ctypes

from nrsc5_amd import engine as eng

STATS = eng.AAS_STATS[:-1]
PSD_PORTS = (0x5100,) + tuple(range(0x5201, 0x5208))


def _i32(x: int) -> int:
    x &= 0xffffffff
    return x - (1 << 32) if x & 0x80000000 else x


def _u32(b, at: int) -> int:
    return b[at] | b[at + 1] << 8 | b[at + 2] << 16 | b[at + 3] << 24


class _File:
    def __init__(self, owner, local, lot):
        self.owner, self.local, self.lot, self.timestamp = owner, local, lot, 0
        self.size = self.mime = 0
        self.expiry = (0, 0, 0, 0, 0)
        self.name = None                                         # as strndup keeps it
        self.bytes_so_far = 0
        self.have = set()
        self.data = bytearray(65536)


class AasModel:
    def __init__(self, lot_files: int = 16, fragments: bool = False):
        self.lot_files, self.fragments = lot_files, fragments
        self.stats = dict.fromkeys(STATS, 0)
        self.reset()

    def reset(self):                                             # aas_reset, output.c:182-202
        self.services = []                                       # [{"type", "number", "name", "comps": [dict]}]; type 1 data, 2 audio
        self.lru = 1
        self.pool = [None] * self.lot_files

    # ---- the table ----
    def flat(self) -> bytes:
        out = bytearray()
        for s in self.services:
            out += bytes((s["type"], s["number"] & 0xff, s["number"] >> 8, len(s["name"]))) + s["name"] + bytes((len(s["comps"]),))
            for c in s["comps"]:
                out += bytes((c["type"], c["id"])) + c["port"].to_bytes(2, "little") + c["sdt"].to_bytes(2, "little") + bytes((c["data_type"],)) + c["mime"].to_bytes(4, "little")
        return bytes(out)

    def sig(self) -> list:
        return eng.aas_sig_table(self.flat())

    def _emit(self, out, kind, port, seq, v, data=b""):
        v = [_i32(x) for x in v] + [0] * (8 - len(v))
        out.append((kind, port, seq, v, bytes(data)))
        self.stats["events"] += 1

    # ---- output_aas_push ----
    def push(self, port: int, seq: int, data: bytes, program: int = 0) -> list:
        out, st = [], self.stats
        st["packets"] += 1
        if port in PSD_PORTS:
            st["psd"] += 1
            self._emit(out, "psd", port, seq, [program], data)
        elif port == 0x20:
            self._sig(out, data)
        elif 0x401 <= port <= 0x50FF:
            self._port(out, port, seq, data)
        else:
            st["unknown_port"] += 1
        return out

    def _sig(self, out, buf):
        st = self.stats
        st["sig_packets"] += 1
        if self.services:
            return
        st["sig_parsed"] += 1
        self._sig_walk(buf)
        if not self.services:
            st["sig_empty"] += 1
        self._emit(out, "sig", 0x20, 0, [len(self.services)], self.flat())

    def _sig_walk(self, buf):
        st, n, p, service = self.stats, len(buf), 0, None
        while p < n:
            t = buf[p]
            p += 1
            if t & 0xF0 == 0x40:
                if p + 2 > n:
                    st["sig_truncated"] += 1
                    return
                number = buf[p] | buf[p + 1] << 8
                idx = next((k for k, s in enumerate(self.services) if s["number"] == number), len(self.services))
                if idx == 16:
                    return
                service = {"type": 2 if t == 0x40 else 1, "number": number, "name": b"", "comps": []}
                if idx < len(self.services):
                    self.services[idx] = service
                else:
                    self.services.append(service)
                p += 3
            elif t & 0xF0 == 0x60:
                if p >= n:
                    st["sig_truncated"] += 1
                    return
                l = buf[p]
                p += 1
                if service is None:
                    return
                if l == 0:
                    st["sig_zero_length"] += 1
                    return
                if t == 0x69:
                    if l < 2 or p + 1 + (l - 2) > n:
                        st["sig_truncated"] += 1
                        return
                    service["name"] = bytes(buf[p + 1:p + 1 + l - 2])
                elif t in (0x67, 0x66):
                    if p + (12 if t == 0x67 else 11) > n:
                        st["sig_truncated"] += 1
                        return
                    cid = buf[p]
                    ci = next((k for k, c in enumerate(service["comps"]) if c["id"] == cid), len(service["comps"]))
                    if ci == 8:
                        return
                    if t == 0x67:
                        c = {"type": 1, "id": cid, "port": buf[p + 1] | buf[p + 2] << 8, "sdt": buf[p + 3] | buf[p + 4] << 8, "data_type": buf[p + 5], "mime": _u32(buf, p + 8)}
                    else:
                        c = {"type": 2, "id": cid, "port": buf[p + 1], "sdt": 0, "data_type": buf[p + 2], "mime": _u32(buf, p + 7)}
                    if ci < len(service["comps"]):
                        service["comps"][ci] = c
                    else:
                        service["comps"].append(c)
                p += l - 1
            else:
                return

    # ---- process_port ----
    def _port(self, out, port, seq, buf):
        st = self.stats
        if not self.services:
            st["before_sig"] += 1
            return
        found = next(((si, ci, c) for si, s in enumerate(self.services) for ci, c in enumerate(s["comps"]) if c["type"] == 1 and c["port"] == port), None)
        if found is None:
            st["not_in_sig"] += 1
            return
        si, ci, c = found
        if c["data_type"] in (0, 1):
            kind = "stream" if c["data_type"] == 0 else "packet"
            self._emit(out, kind, port, seq, [c["mime"], si, ci], buf)
            st[kind] += 1
        elif c["data_type"] == 3:
            self._lot(out, si * 8 + ci, port, buf)
        else:
            st["unknown_type"] += 1

    def _lot(self, out, comp, port, buf):
        st, n = self.stats, len(buf)
        st["lot_packets"] += 1
        if n < 8:
            st["lot_dropped"] += 1
            return
        hdrlen, repeat, lot, seq = buf[0], buf[1], buf[2] | buf[3] << 8, _u32(buf, 4)
        if hdrlen < 8 or hdrlen > n:
            st["lot_dropped"] += 1
            return
        buf, n, hdrlen = buf[8:], n - 8, hdrlen - 8
        if seq >= 256:
            st["lot_dropped"] += 1
            return
        live = [(k, f) for k, f in enumerate(self.pool) if f is not None and f.owner == comp]
        f = next((f for _, f in live if f.lot == lot), None)
        if f is None:
            used = {g.local for _, g in live}
            if len(used) < 12:
                local = min(set(range(12)) - used)
                free = [k for k, g in enumerate(self.pool) if g is None]
                if free:
                    slot = free[0]
                else:
                    slot = min(range(self.lot_files), key=lambda k: (self.pool[k].timestamp, k))
                    st["pool_evictions"] += 1
            else:
                slot, g = min(live, key=lambda kg: (kg[1].timestamp, kg[1].local))
                local = g.local
                st["lru_evictions"] += 1
            f = self.pool[slot] = _File(comp, local, lot)
        f.timestamp = self.lru
        self.lru += 1
        new_data = False
        if hdrlen > 0:
            if hdrlen < 16:
                st["lot_short_header"] += 1
                return
            expiry = ((buf[7] << 4 | buf[6] >> 4) - 1900, (buf[6] & 0xf) - 1, buf[5] >> 3, (buf[5] & 7) << 2 | buf[4] >> 6, buf[4] & 0x3f)
            size, mime = _u32(buf, 8), _u32(buf, 12)
            buf, n, hdrlen = buf[16:], n - 16, hdrlen - 16
            sent = bytes(buf[:hdrlen])
            if f.name is not None:
                if hdrlen != len(f.name) or sent != f.name or size != f.size or mime != f.mime or expiry != f.expiry:
                    slot = self.pool.index(f)
                    f = self.pool[slot] = _File(comp, f.local, lot)
                    f.timestamp = self.lru
                    st["lot_resets"] += 1
                    new_data = True
            else:
                new_data = True
            f.name, f.size, f.mime, f.expiry = sent.split(b"\0", 1)[0], size, mime, expiry
            buf, n = buf[hdrlen:], n - hdrlen
            if new_data:
                self._emit(out, "lot_header", port, 0, [lot, size, mime, *expiry], f.name)
                st["lot_headers"] += 1
        dup = seq in f.have
        if not dup:
            new_data = True
            if n > 256:
                st["lot_too_large"] += 1
                return
            f.data[seq * 256:seq * 256 + 256] = bytes(buf) + bytes(256 - n)
            f.have.add(seq)
            f.bytes_so_far += n
        else:
            st["lot_duplicates"] += 1
        st["lot_fragments"] += 1
        if self.fragments:
            self._emit(out, "lot_fragment", port, seq, [lot, repeat, int(dup), n, f.bytes_so_far])
        if not new_data or f.size == 0:
            return
        if f.size > 65536:
            st["lot_oversize"] += 1
            return
        if any(k not in f.have for k in range((f.size + 255) // 256)):
            return
        self._emit(out, "lot", port, len(f.name), [lot, f.size, f.mime, *f.expiry], bytes(f.data[:f.size]) + f.name)
        st["lot_files"] += 1


def run(packets, lot_files: int = 16, fragments: bool = False, model: AasModel | None = None):
    """-> (per packet [event], the model afterwards)"""
    m = model or AasModel(lot_files, fragments)
    return [m.push(*pk) for pk in packets], m


def ref_form(ev):
    """an event as RefAas records the reference's callback; None for what the reference does not report through it (the PSD packets)"""
    kind, port, seq, v, data = ev
    u = lambda x: x & 0xffffffff
    if kind == "psd":
        return None
    if kind == "sig":
        return ("sig", [(s["type"], s["number"], None if s["name"] is None else s["name"].encode(),
                         [(c["type"], c["id"], c["port"], c.get("service_data_type"), c["data_type"], c["mime"]) for c in s["components"]])
                        for s in eng.aas_sig_table(data)])
    if kind == "lot_header":
        return ("lot_header", port, u(v[0]), u(v[1]), u(v[2]), data, tuple(v[3:8]), None)
    if kind == "lot":
        size = len(data) - seq
        return ("lot", port, u(v[0]), u(v[1]), u(v[2]), data[size:], tuple(v[3:8]), data[:size])
    if kind == "lot_fragment":
        return ("lot_fragment", u(v[0]), seq, v[1], v[2], v[3], u(v[4]))
    return (kind, port, seq, len(data), u(v[0]), data)


# ---- the unmodified reference ------------------------------------------------------------------------------------------------------------------------
class _Component(ctypes.Structure):
    pass


class _CData(ctypes.Structure):
    _fields_ = [("port", ctypes.c_uint16), ("service_data_type", ctypes.c_uint16), ("type", ctypes.c_uint8), ("mime", ctypes.c_uint32)]


class _CAudio(ctypes.Structure):
    _fields_ = [("port", ctypes.c_uint8), ("type", ctypes.c_uint8), ("mime", ctypes.c_uint32)]


class _CUnion(ctypes.Union):
    _fields_ = [("data", _CData), ("audio", _CAudio)]


_Component._anonymous_ = ("u",)
_Component._fields_ = [("next", ctypes.POINTER(_Component)), ("type", ctypes.c_uint8), ("id", ctypes.c_uint8), ("u", _CUnion)]       # nrsc5.h:98-122


class _Service(ctypes.Structure):
    pass


_Service._fields_ = [("next", ctypes.POINTER(_Service)), ("type", ctypes.c_uint8), ("number", ctypes.c_uint16), ("name", ctypes.c_char_p),
                     ("components", ctypes.POINTER(_Component)), ("audio_component", ctypes.POINTER(_Component))]                   # nrsc5.h:148-156


class _Tm(ctypes.Structure):                                     # struct tm: the five fields the reference fills
    _fields_ = [("tm_sec", ctypes.c_int), ("tm_min", ctypes.c_int), ("tm_hour", ctypes.c_int), ("tm_mday", ctypes.c_int), ("tm_mon", ctypes.c_int),
                ("tm_year", ctypes.c_int)]


class _Stream(ctypes.Structure):                                 # nrsc5.h:455-472 (stream and packet alike)
    _fields_ = [("port", ctypes.c_uint16), ("seq", ctypes.c_uint16), ("size", ctypes.c_uint), ("mime", ctypes.c_uint32),
                ("data", ctypes.POINTER(ctypes.c_uint8)), ("service", ctypes.c_void_p), ("component", ctypes.c_void_p)]


class _Lot(ctypes.Structure):                                    # nrsc5.h:473-483
    _fields_ = [("port", ctypes.c_uint16), ("lot", ctypes.c_uint), ("size", ctypes.c_uint), ("mime", ctypes.c_uint32), ("name", ctypes.c_char_p),
                ("data", ctypes.POINTER(ctypes.c_uint8)), ("expiry_utc", ctypes.POINTER(_Tm)), ("service", ctypes.c_void_p), ("component", ctypes.c_void_p)]


class _Fragment(ctypes.Structure):                               # nrsc5.h:484-494
    _fields_ = [("lot", ctypes.c_uint), ("seq", ctypes.c_uint), ("repeat", ctypes.c_uint), ("size", ctypes.c_uint), ("bytes_so_far", ctypes.c_uint),
                ("is_duplicate", ctypes.c_int), ("data", ctypes.POINTER(ctypes.c_uint8)), ("service", ctypes.c_void_p), ("component", ctypes.c_void_p)]


class _Sig(ctypes.Structure):
    _fields_ = [("services", ctypes.POINTER(_Service))]


class _Union(ctypes.Union):
    _fields_ = [("stream", _Stream), ("lot", _Lot), ("fragment", _Fragment), ("sig", _Sig), ("room", ctypes.c_uint8 * 256)]


class _Event(ctypes.Structure):                                  # struct nrsc5_event_t, include/nrsc5.h:369-613
    _anonymous_ = ("u",)
    _fields_ = [("event", ctypes.c_uint), ("u", _Union)]


_CALLBACK = ctypes.CFUNCTYPE(None, ctypes.POINTER(_Event), ctypes.c_void_p)
_EV = {9: "sig", 10: "lot", 12: "stream", 13: "packet", 24: "lot_header", 25: "lot_fragment"}        # NRSC5_EVENT_*, include/nrsc5.h:162-195


class RefAas:
    """One session of the unmodified reference (oracle/_ref/libnrsc5_ref.so): nrsc5_open_pipe / nrsc5_set_callback, a ctypes callback that records the SIG /
    LOT_HEADER / LOT_FRAGMENT / LOT / STREAM / PACKET events in ref_form's shape (fragments without their data).  push hands packets to the reference's own
    output_aas_push on an output_t of the test's -- a zeroed buffer of 32 MB, larger than output_t (its elastic buffers take 18.7 MB), set up by the reference's
    own output_init.  run_iq feeds samples through the public API."""

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
        L.output_init.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.output_init.restype = None
        L.output_aas_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
        L.output_aas_push.restype = None
        self.radio = ctypes.c_void_p()
        if L.nrsc5_open_pipe(ctypes.byref(self.radio)) != 0:
            raise RuntimeError("nrsc5_open_pipe failed")
        L.nrsc5_set_mode(self.radio, mode)
        self.events, self._out = [], None
        self._cb = _CALLBACK(self._on_event)
        L.nrsc5_set_callback(self.radio, self._cb, None)

    def _on_event(self, evt, opaque):
        e = evt.contents
        kind = _EV.get(e.event)
        if kind is None:
            return
        raw = lambda p, n: bytes(ctypes.string_at(p, n)) if n else b""
        if kind == "sig":
            table, s = [], e.sig.services
            while s:
                sv, comps, c = s.contents, [], s.contents.components
                while c:
                    cc = c.contents
                    if cc.type == 1:                             # NRSC5_SIG_COMPONENT_DATA
                        comps.append(("data", cc.id, cc.data.port, cc.data.service_data_type, cc.data.type, cc.data.mime))
                    else:
                        comps.append(("audio", cc.id, cc.audio.port, None, cc.audio.type, cc.audio.mime))
                    c = cc.next
                table.append(("data" if sv.type == 1 else "audio", sv.number, sv.name, comps))
                s = sv.next
            r = ("sig", table)
        elif kind in ("lot", "lot_header"):
            t = e.lot.expiry_utc.contents
            r = (kind, e.lot.port, e.lot.lot, e.lot.size, e.lot.mime, e.lot.name, (t.tm_year, t.tm_mon, t.tm_mday, t.tm_hour, t.tm_min),
                 raw(e.lot.data, e.lot.size) if kind == "lot" else None)
        elif kind == "lot_fragment":
            f = e.fragment
            r = (kind, f.lot, f.seq, f.repeat, f.is_duplicate, f.size, f.bytes_so_far)
        else:
            r = (kind, e.stream.port, e.stream.seq, e.stream.size, e.stream.mime, raw(e.stream.data, e.stream.size))
        self.events.append(r)

    def push(self, packets) -> list:
        """-> per packet (port, seq, data[, program]) the events the reference's output_aas_push fired"""
        if self._out is None:
            self._out = ctypes.create_string_buffer(32 << 20)
            self.lib.output_init(self._out, self.radio)
        per = []
        for pk in packets:
            port, seq, data = pk[:3]
            buf = ctypes.create_string_buffer(int(port).to_bytes(2, "little") + int(seq).to_bytes(2, "little") + bytes(data), 4 + len(data) + 16)
            first = len(self.events)
            self.lib.output_aas_push(self._out, buf, 4 + len(data))
            per.append(self.events[first:])
        return per

    def run_iq(self, iq, chunk: int = 32768) -> list:
        import numpy as np
        iq = np.ascontiguousarray(iq)
        push = self.lib.nrsc5_pipe_samples_cu8 if iq.dtype == np.uint8 else self.lib.nrsc5_pipe_samples_cs16
        for off in range(0, iq.size, chunk):
            part = iq[off:off + chunk]
            push(self.radio, part.ctypes.data, part.size)
        return self.events

    def close(self):
        if self.radio:
            self.lib.nrsc5_close(self.radio)
            self.radio = ctypes.c_void_p()
