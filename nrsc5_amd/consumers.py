"""The consumers of an engine's block records (nrsc5hip_hdc_* / _psd_* / _sis_* / _aas_*): audio packets on the host, PSD packets, SIS events and
data-service events (SIG, LOT files) from their arenas on the device.  Every name here is reachable as nrsc5_amd.engine.<name> too."""
from __future__ import annotations

import ctypes
import numpy as np

from .abi import (AAS_CB, AAS_EVENT_CB, AAS_FRAGMENTS, AAS_KINDS, AAS_SIG_MAX, AAS_STATS, HDC_CB, L2_AM, L2_FM_P1, L2_FM_PX, MODE_FM, PSD_STATS, REC_PROCESSED, REC_TO_FINE, RECORD_DTYPE, SIS_CB, SIS_KINDS, SIS_STATS,
                  L2Frame, Nrsc5HipError, SisInfo)


def _record_args(recs_per_stream):
    """-> (the RECORD_DTYPE arrays, to be kept alive over the call; their pointers; their lengths): None and empty arrays as null pointers"""
    arrs = [None if r is None else np.ascontiguousarray(r, dtype=RECORD_DTYPE) for r in recs_per_stream]
    ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[None if a is None or a.size == 0 else a.ctypes.data for a in arrs])
    return arrs, ptrs, np.array([0 if a is None else a.size for a in arrs], dtype=np.int32)


def _ids_targets(stream_ids, targets, recs_per_stream):
    ids = np.ascontiguousarray(stream_ids, dtype=np.int32).reshape(-1)
    tg = None if targets is None else np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
    if len(recs_per_stream) != ids.size or (tg is not None and tg.size != ids.size):
        raise ValueError("stream_ids, recs_per_stream and targets must have one entry per stream")
    return ids, tg


class _Consumer:
    """The life cycle of a native consumer handle (self.lib, self._h; _destroy: the name of its destroy function) and what its calls have in common"""
    _destroy = None

    def _result(self, rc: int, what: str) -> int:
        if rc < 0:
            err = Nrsc5HipError(f"{what} failed ({rc}): {self.lib.nrsc5hip_last_error().decode()}")
            err.code = rc
            raise err
        return rc

    def _appended(self, out: list, what: str, *args) -> list:
        """runs self.lib.<what>(*args), which reports through the callback into `out` and returns how many times; -> what it appended"""
        first = len(out)
        rc = self._result(getattr(self.lib, what)(*args), what)
        got = out[first:]
        assert rc == len(got)
        return got

    def _stats(self, what: str, names, stream: int) -> dict:
        v = (ctypes.c_longlong * len(names))()
        self._result(getattr(self.lib, what)(self._h, stream, v), what)
        return dict(zip(names, (int(x) for x in v)))

    def _create(self, what: str, engine, nstreams: int):
        """a consumer whose device buffers live on the engine's device: keeps the engine alive"""
        self.lib, self._engine, self._h, self.nstreams = engine.lib, engine, ctypes.c_void_p(), nstreams
        rc = getattr(self.lib, what)(engine._h, nstreams, ctypes.byref(self._h))
        if rc != 0:
            raise Nrsc5HipError(f"{what} failed ({rc}): {self.lib.nrsc5hip_last_error().decode()}")

    def close(self):
        if self._h:
            getattr(self.lib, self._destroy)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HdcConsumer(_Consumer):
    """Slim batch consumer of the L2 index (nrsc5hip_hdc_*): elastic buffers of `nstreams` streams in ~40 KB each instead of
    one nrsc5_t per stream; delivers the reference's NRSC5_EVENT_HDC sequence."""
    _destroy = "nrsc5hip_hdc_destroy"

    def __init__(self, nstreams: int, lib: ctypes.CDLL | None = None, lib_path: str | None = None):
        if lib is None:
            from .engine import load_library                     # (here, not at the top: engine imports this module)
            lib = load_library(lib_path)
        self.lib = lib
        self._h = ctypes.c_void_p()
        if self.lib.nrsc5hip_hdc_create(nstreams, ctypes.byref(self._h)) != 0:
            raise Nrsc5HipError("nrsc5hip_hdc_create failed")
        self.events = []
        self._cb = HDC_CB(self._on_packet)

    def _on_packet(self, opaque, stream, program, data, count, flags):
        self.events.append((int(stream), int(program), int(count), int(flags), bytes(ctypes.string_at(data, count)) if count else b""))

    def push_frame(self, stream: int, frame: L2Frame, pdu_bytes: np.ndarray, lc: int = 0):
        b = np.ascontiguousarray(pdu_bytes, dtype=np.uint8)
        if self.lib.nrsc5hip_hdc_push_frame(self._h, stream, lc, ctypes.byref(frame), b.ctypes.data) != 0:
            raise Nrsc5HipError("nrsc5hip_hdc_push_frame failed")

    def fixed_audio_end(self, stream: int, lc: int, pdu_bytes: np.ndarray) -> int:
        b = np.ascontiguousarray(pdu_bytes, dtype=np.uint8)
        return int(self.lib.nrsc5hip_hdc_fixed_audio_end(self._h, stream, lc, b.ctypes.data, b.size))

    def frame_reset(self, stream: int):
        self.lib.nrsc5hip_hdc_frame_reset(self._h, stream)

    def advance(self, stream: int, mode: int = MODE_FM) -> int:
        return self.lib.nrsc5hip_hdc_advance(self._h, stream, mode, self._cb, None)

    def reset(self, stream: int):
        self.lib.nrsc5hip_hdc_reset(self._h, stream)

    def host_bytes(self) -> int:
        return int(self.lib.nrsc5hip_hdc_host_bytes(self._h))

    def adts(self, data: bytes) -> bytes:
        out = (ctypes.c_uint8 * (len(data) + 7))()
        src = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        n = self.lib.nrsc5hip_hdc_adts(src, len(data), out)
        return bytes(out[:n])


def feed_hdc(engine, consumer: HdcConsumer, stream: int, recs: np.ndarray, mode: int = MODE_FM, target_stream: int | None = None):
    """Replays one stream's block records into the consumer in the reference's order: output_advance at the top of every
    processed block (acquire.c:108), then the frames that block delivers (frame_push -> frame_process)."""
    from .engine import l2_jobs_from_records
    t = stream if target_stream is None else target_stream
    jobs_all = []
    per_rec = []
    for r in recs:
        jobs = l2_jobs_from_records(stream, np.array([r], dtype=RECORD_DTYPE), mode)
        per_rec.append((len(jobs_all), len(jobs)))
        jobs_all += jobs
    frames, by = engine.l2_index_raw(jobs_all) if jobs_all else (None, None)
    for r, (first, n) in zip(recs, per_rec):
        if int(r["flags"]) & REC_PROCESSED:
            consumer.advance(t, mode)
        if int(r["flags"]) & REC_TO_FINE:
            consumer.frame_reset(t)                              # sync.c:405-409
        for k in range(first, first + n):
            kind, which = jobs_all[k][2], jobs_all[k][3]
            lc = 0 if kind == L2_FM_P1 or (kind == L2_AM and which < 8) else (1 + which if kind == L2_FM_PX else 1)
            consumer.push_frame(t, frames[k], by[k, :frames[k].nbytes], lc)


def feed_hdc_batch(engine, consumer: HdcConsumer, stream_ids, recs_per_stream, mode: int = MODE_FM, targets=None) -> int:
    """nrsc5hip_hdc_feed: what feed_hdc does, for many streams in one native call -- one L2 index launch and one copy for all their
    frames, no Python per record.  recs_per_stream[i]: the RECORD_DTYPE array of engine stream stream_ids[i] (drained since the last
    call; may be empty); targets[i]: the consumer's stream for it (None: the same ids).  The packets land in consumer.events, all of
    stream_ids[0] first; -> how many.  Call it while the ring slots the records name still hold their frames."""
    ids, tg = _ids_targets(stream_ids, targets, recs_per_stream)
    arrs, ptrs, counts = _record_args(recs_per_stream)
    return consumer._result(consumer.lib.nrsc5hip_hdc_feed(consumer._h, engine._h, int(ids.size), ids.ctypes.data, None if tg is None else tg.ctypes.data, ptrs,
                                                           counts.ctypes.data, mode, consumer._cb, None), "nrsc5hip_hdc_feed")


class PsdConsumer(_Consumer):
    """PSD transport on the device (nrsc5hip_psd_*): HDLC de-framing of the PSD spans of `nstreams` streams in HBM; only finished AAS
    packets reach the host.  They land in `packets` as (stream, program, port, seq, data), data = what follows port and seq."""
    _destroy = "nrsc5hip_psd_destroy"

    def __init__(self, engine, nstreams: int):
        self._create("nrsc5hip_psd_create", engine, nstreams)
        self.packets = []
        self._cb = AAS_CB(self._on_packet)

    def _on_packet(self, opaque, stream, program, port, seq, data, n):
        self.packets.append((int(stream), int(program), int(port), int(seq), bytes(ctypes.string_at(data, n)) if n else b""))

    def reset(self, stream: int):
        self._result(self.lib.nrsc5hip_psd_reset(self._h, stream), "nrsc5hip_psd_reset")

    def stats(self, stream: int) -> dict:
        return self._stats("nrsc5hip_psd_stats", PSD_STATS, stream)

    def stage(self, stream: int, frames_bits: np.ndarray, lc: int = 0) -> int:
        """nrsc5hip_stage_psd: frames as frame_push takes them ([nframes, nbits], one bit per byte), in order; -> packets delivered"""
        b = np.ascontiguousarray(frames_bits, dtype=np.uint8)
        if b.ndim == 1:
            b = b[None, :]
        return self._result(self.lib.nrsc5hip_stage_psd(self._h, self._engine._h, stream, b.ctypes.data, b.shape[1], b.shape[0], lc, self._cb, None),
                            "nrsc5hip_stage_psd")

    def stage_streams(self, targets, frames_per_stream, lcs, reset_at=None) -> list:
        """nrsc5hip_stage_psd_streams: frames_per_stream[i] ([nframes, nbits] bits) go to consumer stream targets[i], all in one call (one k_psd
        workgroup per stream); reset_at[i]: the frame in front of which the stream gets a REC_TO_FINE reset (None / negative: none).
        -> the packets of this call, all of targets[0] first"""
        n = len(targets)
        arrs = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames_per_stream]
        arrs = [a[None, :] if a.ndim == 1 else a for a in arrs]
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        tg, nb, nf, lc = i32(targets), i32([a.shape[1] for a in arrs]), i32([a.shape[0] for a in arrs]), i32(lcs)
        rs = None if reset_at is None else i32([-1 if r is None else r for r in reset_at])
        ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        return self._appended(self.packets, "nrsc5hip_stage_psd_streams", self._h, self._engine._h, n, tg.ctypes.data, ptrs, nb.ctypes.data, nf.ctypes.data,
                              lc.ctypes.data, None if rs is None else rs.ctypes.data, self._cb, None)


def feed_psd_batch(engine, consumer: PsdConsumer, stream_ids, recs_per_stream, targets=None, mode: int = MODE_FM) -> list:
    """nrsc5hip_psd_feed: the records of many streams (as for feed_hdc_batch) replayed into the PSD consumer in one native call -- one
    index launch, one k_psd launch, one copy of the finished packets.  -> [(stream, program, port, seq, data)] of this call, all of
    stream_ids[0] first (they are appended to consumer.packets as well).  Call it while the ring slots the records name hold their frames."""
    ids, tg = _ids_targets(stream_ids, targets, recs_per_stream)
    arrs, ptrs, counts = _record_args(recs_per_stream)
    return consumer._appended(consumer.packets, "nrsc5hip_psd_feed", consumer._h, engine._h, int(ids.size), ids.ctypes.data, None if tg is None else tg.ctypes.data,
                              ptrs, counts.ctypes.data, mode, consumer._cb, None)


def sis_utf8(enc: int, data: bytes) -> bytes | None:
    """The C string the reference reports for `data` in encoding `enc` (utf8_encode, pids.c:272-282; unicode.c): 0 = ISO-8859-1, 4 = UCS-2 with an
    optional byte-order mark (little endian without one; an odd last byte is dropped); any other encoding gives None (a NULL string).  The result is
    cut at its first NUL, as a C string is.  (UCS-2 of length 0 is "": the reference's loop bound wraps there.)"""
    data = bytes(data)
    if enc == 0:
        out = data.decode("latin-1").encode("utf-8")
    elif enc == 4:
        big = data[:2] == b"\xfe\xff"
        body = data[2:] if data[:2] in (b"\xfe\xff", b"\xff\xfe") else data
        body = body[:len(body) - len(body) % 2]
        out = bytearray()
        for k in range(0, len(body), 2):
            ch = (body[k] << 8 | body[k + 1]) if big else (body[k] | body[k + 1] << 8)
            if ch < 0x80:
                out.append(ch)
            elif ch < 0x800:
                out += bytes((0xc0 | ch >> 6, 0x80 | ch & 0x3f))
            else:
                out += bytes((0xe0 | ch >> 12, 0x80 | (ch >> 6) & 0x3f, 0x80 | ch & 0x3f))     # (surrogates too: the reference does not pair them)
        out = bytes(out)
    else:
        return None
    return out.split(b"\0", 1)[0]


def sis_text(enc: int, data: bytes) -> str | None:
    raw = sis_utf8(enc, data)
    return None if raw is None else raw.decode("utf-8", errors="replace")


def rds_text(data: bytes) -> str:
    """RDS name or RadioText for display: 0x20 .. 0x7E as ASCII, any other byte as U+FFFD; trailing spaces and the 0x0D that ends a text cut"""
    data = bytes(data)
    if b"\r" in data:
        data = data[:data.index(b"\r")]
    return "".join(chr(b) if 0x20 <= b <= 0x7E else "\ufffd" for b in data).rstrip(" ")


def rds_callsign(pi: int) -> str | None:
    """the RBDS rule: PI 0x1000 .. 0x54A7 is K + three letters in base 26, 0x54A8 .. 0x994F is W + three letters; anything else has no call sign"""
    if 0x1000 <= pi <= 0x54A7:
        first, n = "K", pi - 0x1000
    elif 0x54A8 <= pi <= 0x994F:
        first, n = "W", pi - 0x54A8
    else:
        return None
    return first + "".join(chr(65 + n // k % 26) for k in (676, 26, 1))


def rds_event_fields(kind: str, v, data: bytes) -> dict:
    """An event of k_rds_groups as named fields; text decoded by rds_text, the raw bytes beside it"""
    if kind == "pi":
        return {"pi": v[0], "callsign": rds_callsign(v[0])}
    if kind == "ps":
        return {"pi": v[0], "ps": rds_text(data), "raw": bytes(data)}
    if kind == "rt":
        return {"pi": v[0], "ab": v[1], "text": rds_text(data), "raw": bytes(data)}
    if kind == "clock":
        return {"mjd": v[0], "hour": v[1], "minute": v[2], "offset_half_hours": v[3]}
    if kind == "group":
        return {"blocks": tuple(v[:4])}
    raise ValueError(kind)


def same_fields(text) -> dict | None:
    """A SAME header ZCZC-ORG-EEE-PSSCCC(-PSSCCC ..)+TTTT-JJJHHMM-LLLLLLLL- as named fields: originator, event code, the location codes, purge time
    in minutes (TTTT is hours and minutes), issue day of the year / hour / minute (UTC) and the sender; None for text that does not have the form
    (the end of message NNNN included)"""
    import re
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode("latin-1")
    m = re.fullmatch(r"ZCZC-([A-Z]{3})-([A-Z0-9]{3})((?:-[0-9]{6}){1,31})\+([0-9]{4})-([0-9]{3})([0-9]{2})([0-9]{2})-([\x20-\x2c\x2e-\x7e]{8})-", text)
    if not m:
        return None
    purge = int(m.group(4))
    return {"originator": m.group(1), "event": m.group(2), "locations": m.group(3)[1:].split("-"), "purge_minutes": 60 * (purge // 100) + purge % 100,
            "day": int(m.group(5)), "hour": int(m.group(6)), "minute": int(m.group(7)), "sender": m.group(8).rstrip(" ")}


def same_event_fields(kind: str, v, data: bytes) -> dict:
    """An event of k_same_frames as named fields: the text, its kind ("header" / "eom"), for a header its same_fields (None when it has not the
    form), and the burst's place in its group / the bursts the group had when the message was decided"""
    from .abi import SAME_BURST_KINDS
    text = bytes(data).decode("latin-1")
    out = {"text": text, "kind": SAME_BURST_KINDS[v[0]], "fields": same_fields(text) if v[0] == 1 else None, "bursts": v[1]}
    if kind == "burst":
        out["preamble_bits"] = v[2]
    elif kind != "message":
        raise ValueError(kind)
    return out


def same_line(text) -> str:
    """what the command line prints for a message: `EAS WXR TOR 029095,029097 +0030 day 123 14:05 KXYZ/FM`, `EAS end of message`"""
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode("latin-1")
    if text == "NNNN":
        return "EAS end of message"
    f = same_fields(text)
    if f is None:
        return "EAS " + text
    return "EAS %s %s %s +%02d%02d day %03d %02d:%02d %s" % (f["originator"], f["event"], ",".join(f["locations"]), f["purge_minutes"] // 60,
                                                             f["purge_minutes"] % 60, f["day"], f["hour"], f["minute"], f["sender"])


def _sis_device_info(p) -> dict:
    """manufacturer id, versions and status of parameters 4..7 / 8..11 (pids.c:698-744)"""
    ver = lambda a, b: [(a >> 11) & 0x1f, (a >> 6) & 0x1f, (a >> 1) & 0x1f, b]
    return {"manufacturer_id": bytes(((p[0] >> 8) & 0x7f, p[0] & 0x7f)).split(b"\0", 1)[0].decode("latin-1"),
            "core_version": ver(p[1], (p[3] >> 11) & 0x1f), "manufacturer_version": ver(p[2], (p[3] >> 6) & 0x1f),
            "core_status": (p[3] >> 3) & 7, "manufacturer_status": p[3] & 7}


def sis_event_fields(kind: str, v, enc: int, data: bytes) -> dict:
    """An event of k_sis as the fields the reference's callback reports; text as sis_text gives it (None: an encoding the reference cannot convert)"""
    if kind == "station_id":
        return {"country": data.decode("latin-1"), "fcc": v[0]}
    if kind == "station_name":
        return {"name": sis_text(enc, data)}
    if kind == "station_slogan":
        return {"slogan": sis_text(enc, data)}
    if kind == "station_message":
        return {"message": sis_text(enc, data), "priority": v[0]}
    if kind == "station_location":
        return {"latitude": float(np.float32(v[0]) / np.float32(8192)), "longitude": float(np.float32(v[1]) / np.float32(8192)), "altitude": v[2]}
    if kind == "audio_service":
        return {"program": v[0], "access": v[1], "type": v[2], "sound_exp": v[3]}
    if kind == "data_service":
        return {"access": v[0], "type": v[1], "mime_type": v[2]}
    if kind == "alert":
        if v[0] < 0:
            return {"message": None, "control_data": None}
        return {"message": sis_text(enc, data[v[0]:]), "control_data": data[:v[0]]}
    if kind == "leap_second":
        return {"pending_offset": v[0], "current_offset": v[1], "pending_alfn": v[2] & 0xffffffff}
    if kind == "local_time":
        return {"utc_offset": v[0], "dst_regional": v[1], "dst_local": v[2], "dst_schedule": v[3]}
    if kind == "exciter":
        return {**_sis_device_info(v), "importer_connected": (v[0] >> 7) & 1}
    if kind == "importer":
        return _sis_device_info(v)
    raise ValueError(kind)


class SisConsumer(_Consumer):
    """SIS on the device (nrsc5hip_sis_*): pids_frame_push / sis_decode over the PIDS frames of `nstreams` streams, their state in HBM; only
    events reach the host.  They land in `events` as (stream, frame, kind, fields) -- frame: index of the firing frame in the stream's list of
    that call -- and, raw, in `raw` as (stream, frame, kind, v[8], enc, data)."""
    _destroy = "nrsc5hip_sis_destroy"

    def __init__(self, engine, nstreams: int):
        self._create("nrsc5hip_sis_create", engine, nstreams)
        self.events, self.raw = [], []
        self._cb = SIS_CB(self._on_event)

    def _on_event(self, opaque, stream, frame, kind, v, enc, data, n):
        vals, body = [int(v[k]) for k in range(8)], bytes(ctypes.string_at(data, n)) if n else b""
        name = SIS_KINDS[kind]
        self.raw.append((int(stream), int(frame), name, vals, int(enc), body))
        self.events.append((int(stream), int(frame), name, sis_event_fields(name, vals, int(enc), body)))

    def reset(self, stream: int):
        self._result(self.lib.nrsc5hip_sis_reset(self._h, stream), "nrsc5hip_sis_reset")

    def stats(self, stream: int) -> dict:
        return self._stats("nrsc5hip_sis_stats", SIS_STATS, stream)

    def info(self, stream: int) -> dict:
        """nrsc5hip_sis_get: the snapshot, i.e. what the reference's aggregated SIS event would hold"""
        s = SisInfo()
        self._result(self.lib.nrsc5hip_sis_get(self._h, stream, ctypes.byref(s)), "nrsc5hip_sis_get")
        text = lambda enc, buf, n: None if n < 0 else sis_text(enc, bytes(buf[:n]))
        return {"country": s.country_code.decode("latin-1") or None, "fcc": s.fcc_facility_id,
                "name": text(s.name_enc, s.name, s.name_len), "slogan": text(s.slogan_enc, s.slogan, s.slogan_len),
                "message": text(s.message_enc, s.message, s.message_len),
                "alert": None if s.alert_len < 0 else sis_text(s.alert_enc, bytes(s.alert[s.alert_cnt_len:s.alert_len])),
                "alert_control_data": None if s.alert_len < 0 else bytes(s.alert[:s.alert_cnt_len]),
                "location": None if not s.have_location else (float(np.float32(s.latitude) / np.float32(8192)),
                                                                float(np.float32(s.longitude) / np.float32(8192)), s.altitude),
                "audio_services": [tuple(s.audio[k]) for k in range(s.n_audio)], "data_services": [tuple(s.data[k]) for k in range(s.n_data)]}

    def debug_arena(self, nbytes: int):
        self._result(self.lib.nrsc5hip_sis_debug_arena(self._h, nbytes), "nrsc5hip_sis_debug_arena")

    def stage(self, targets, frames_per_stream, reset_at=None) -> list:
        """nrsc5hip_stage_sis: frames_per_stream[i] ([nframes, 80] bits as handed to pids_frame_push; may be empty) go to consumer stream targets[i],
        all in one call (one k_sis workgroup per stream); reset_at[i]: the frame in front of which the stream's state is reset (None / negative:
        none; == nframes: behind the last).  -> the events of this call, all of targets[0] first"""
        n = len(targets)
        arrs = [np.ascontiguousarray(f, dtype=np.uint8).reshape(-1, 80) for f in frames_per_stream]
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        tg, nf = i32(targets), i32([a.shape[0] for a in arrs])
        rs = None if reset_at is None else i32([-1 if r is None else r for r in reset_at])
        ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
        return self._appended(self.events, "nrsc5hip_stage_sis", self._h, n, tg.ctypes.data, ptrs, nf.ctypes.data, None if rs is None else rs.ctypes.data,
                              self._cb, None)


def feed_sis_batch(sis: SisConsumer, targets, fresh) -> list:
    """nrsc5hip_sis_feed: the records of many streams (fresh[i]: the RECORD_DTYPE array for consumer stream targets[i], FM or AM; may be empty or None)
    in one native call -- one upload of 16 bytes per record, one k_sis launch, one copy of the events.  -> [(stream, frame, kind, fields)] of this
    call, all of targets[0] first (they are appended to sis.events as well)."""
    tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
    if len(fresh) != tg.size:
        raise ValueError("targets and fresh must have one entry per stream")
    arrs, ptrs, counts = _record_args(fresh)
    return sis._appended(sis.events, "nrsc5hip_sis_feed", sis._h, int(tg.size), tg.ctypes.data, ptrs, counts.ctypes.data, sis._cb, None)


def aas_sig_table(data: bytes) -> list:
    """The flat SIG layout of include/nrsc5hip.h (the SIG event's data, nrsc5hip_aas_sig) as a list of services with their components, as the
    reference's NRSC5_EVENT_SIG lists them; the name converted like the reference's (ISO-8859-1 -> UTF-8, cut at a NUL), None where none was sent"""
    out, p = [], 0
    while p < len(data):
        kind, number, n = data[p], data[p + 1] | data[p + 2] << 8, data[p + 3]
        name = sis_text(0, data[p + 4:p + 4 + n]) if n else None
        p += 4 + n
        comps = []
        for _ in range(data[p]):
            c = data[p + 1:p + 12]
            comp = {"type": "audio" if c[0] == 2 else "data", "id": c[1], "port": c[2] | c[3] << 8}
            if c[0] == 1:
                comp["service_data_type"] = c[4] | c[5] << 8
            comp["data_type"] = c[6]
            comp["mime"] = int.from_bytes(c[7:11], "little")
            comps.append(comp)
            p += 11
        p += 1
        out.append({"type": "audio" if kind == 2 else "data", "number": number, "name": name, "components": comps})
    return out


def aas_event_fields(kind: str, port: int, seq: int, v, data: bytes):
    """An event of k_aas as the fields the reference's callback reports (nrsc5.h: sig, lot, lot_fragment, stream, packet); "psd" is the packet for the
    ID3 parser.  A sig event is the list of services; names of files as str (ISO-8859-1)"""
    if kind == "psd":
        return {"program": v[0], "port": port, "seq": seq, "data": data}
    if kind == "sig":
        return aas_sig_table(data)
    if kind in ("lot_header", "lot"):
        f = {"port": port, "lot": v[0], "size": v[1] & 0xffffffff, "mime": v[2] & 0xffffffff, "expiry": tuple(v[3:8])}
        if kind == "lot":
            size = len(data) - seq
            f["name"], f["data"] = data[size:].decode("latin-1"), data[:size]
        else:
            f["name"] = data.decode("latin-1")
        return f
    if kind == "lot_fragment":
        return {"port": port, "lot": v[0], "seq": seq, "repeat": v[1], "is_duplicate": v[2], "size": v[3], "bytes_so_far": v[4] & 0xffffffff}
    if kind in ("stream", "packet"):
        return {"port": port, "seq": seq, "mime": v[0] & 0xffffffff, "service": v[1], "component": v[2], "data": data}
    raise ValueError(kind)


def aas_packets(packets) -> np.ndarray:
    """[(port, seq, data) or (port, seq, data, program)] as nrsc5hip_stage_aas takes a stream's packets"""
    out = bytearray()
    for pk in packets:
        port, seq, data = pk[:3]
        out += int(port).to_bytes(2, "little") + int(seq).to_bytes(2, "little") + len(data).to_bytes(2, "little") + (pk[3] if len(pk) > 3 else 0).to_bytes(2, "little")
        out += bytes(data)
    return np.frombuffer(bytes(out), dtype=np.uint8)


class AasConsumer(_Consumer):
    """Data services on the device (nrsc5hip_aas_*), chained behind a PsdConsumer: SIG, port routing and LOT reassembly over the packet arena in HBM;
    only events reach the host.  They land in `events` as (stream, kind, fields) and, raw, in `raw` as (stream, kind, port, seq, v[8], data).
    lot_files: file slots per stream (1..64); fragments: write LOT_FRAGMENT events (they never carry the fragment's bytes)."""
    _destroy = "nrsc5hip_aas_destroy"

    def __init__(self, engine, nstreams: int, lot_files: int = 16, fragments: bool = False):
        self.lib, self._engine, self._h, self.nstreams, self.lot_files = engine.lib, engine, ctypes.c_void_p(), nstreams, lot_files
        rc = self.lib.nrsc5hip_aas_create(engine._h, nstreams, lot_files, AAS_FRAGMENTS if fragments else 0, ctypes.byref(self._h))
        if rc != 0:
            raise Nrsc5HipError(f"nrsc5hip_aas_create failed ({rc}): {self.lib.nrsc5hip_last_error().decode()}")
        self.events, self.raw = [], []
        self._cb = AAS_EVENT_CB(self._on_event)

    def _on_event(self, opaque, stream, kind, port, seq, v, data, n):
        vals, body, name = [int(v[k]) for k in range(8)], bytes(ctypes.string_at(data, n)) if n else b"", AAS_KINDS[kind]
        self.raw.append((int(stream), name, int(port), int(seq), vals, body))
        self.events.append((int(stream), name, aas_event_fields(name, int(port), int(seq), vals, body)))

    def reset(self, stream: int):
        self._result(self.lib.nrsc5hip_aas_reset(self._h, stream), "nrsc5hip_aas_reset")

    def stats(self, stream: int) -> dict:
        return self._stats("nrsc5hip_aas_stats", AAS_STATS, stream)

    def sig(self, stream: int) -> list:
        """nrsc5hip_aas_sig: the stream's SIG table as the sig event held it ([] while no SIG has been seen)"""
        out, n, ns = (ctypes.c_uint8 * AAS_SIG_MAX)(), ctypes.c_uint(), ctypes.c_int()
        self._result(self.lib.nrsc5hip_aas_sig(self._h, stream, out, ctypes.byref(n), ctypes.byref(ns)), "nrsc5hip_aas_sig")
        table = aas_sig_table(bytes(out[:n.value]))
        assert len(table) == ns.value
        return table

    def debug_arena(self, nbytes: int):
        self._result(self.lib.nrsc5hip_aas_debug_arena(self._h, nbytes), "nrsc5hip_aas_debug_arena")

    def stage(self, targets, packets_per_stream) -> list:
        """nrsc5hip_stage_aas: packets_per_stream[i] ([(port, seq, data[, program])], may be empty) go to consumer stream targets[i], all in one call
        (one k_aas workgroup per stream).  -> the events of this call, all of targets[0] first"""
        n = len(targets)
        arrs = [aas_packets(p) for p in packets_per_stream]
        tg, nb = np.ascontiguousarray(targets, dtype=np.int32), np.ascontiguousarray([a.size for a in arrs], dtype=np.int32)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
        return self._appended(self.events, "nrsc5hip_stage_aas", self._h, n, tg.ctypes.data, ptrs, nb.ctypes.data, self._cb, None)

    def stage_frames(self, psd: PsdConsumer, targets, frames_per_stream, lcs, reset_at=None) -> list:
        """nrsc5hip_stage_aas_frames: PsdConsumer.stage_streams with k_aas chained behind k_psd.  -> the events of this call, all of targets[0] first"""
        n = len(targets)
        arrs = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames_per_stream]
        arrs = [a[None, :] if a.ndim == 1 else a for a in arrs]
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        tg, nb, nf, lc = i32(targets), i32([a.shape[1] for a in arrs]), i32([a.shape[0] for a in arrs]), i32(lcs)
        rs = None if reset_at is None else i32([-1 if r is None else r for r in reset_at])
        ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        return self._appended(self.events, "nrsc5hip_stage_aas_frames", self._h, psd._h, self._engine._h, n, tg.ctypes.data, ptrs, nb.ctypes.data,
                              nf.ctypes.data, lc.ctypes.data, None if rs is None else rs.ctypes.data, self._cb, None)


def feed_aas_batch(engine, aas: AasConsumer, psd: PsdConsumer, stream_ids, recs_per_stream, targets=None, mode: int = MODE_FM) -> list:
    """nrsc5hip_aas_feed: feed_psd_batch with the data services chained behind it -- the PSD consumer advances as it would there, its packets stay in
    device memory, one k_aas launch runs over them.  -> [(stream, kind, fields)] of this call, all of stream_ids[0] first (appended to aas.events as
    well); kinds: "psd", "sig", "lot_header", "lot_fragment", "lot", "stream", "packet".  Call it while the ring slots the records name hold their frames."""
    ids, tg = _ids_targets(stream_ids, targets, recs_per_stream)
    arrs, ptrs, counts = _record_args(recs_per_stream)
    return aas._appended(aas.events, "nrsc5hip_aas_feed", aas._h, psd._h, engine._h, int(ids.size), ids.ctypes.data, None if tg is None else tg.ctypes.data,
                         ptrs, counts.ctypes.data, mode, aas._cb, None)
