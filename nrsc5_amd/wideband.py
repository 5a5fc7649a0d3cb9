"""Decode every listed HD station of one wideband SDR capture: the channelizer (nrsc5hip_chan_*) feeds one engine stream per station,
and the batch engine decodes them (p1_async, l2_feedback).

    python -m nrsc5_amd.wideband FILE --format cs16 --rate 20000000 --offsets -800e3,0,400e3
    rtl_sdr -f 98.1e6 -s 2400000 - | python -m nrsc5_amd.wideband - --format cu8 --rate 2400000 --offsets -800e3,0,600e3

prints one line per station event (SYNC with its frequency offset, MER, BER, LOST_SYNC).  --metadata adds what every program is playing
(one ID3 line per tag: title, artist, album, genre), de-framed on the device (nrsc5hip_psd_feed): no frame is copied to the host for it.
--sis adds who every station is (one line per station id, name, slogan, message, location, service descriptor, alert and time / exciter / importer
parameter as it arrives), decoded from the PIDS frames on the device (nrsc5hip_sis_feed); with a scan, every `found` line then carries the call sign.
--dump-hdc DIR also records every station's
audio programs (the reference's NRSC5_EVENT_HDC packets, as `nrsc5 --dump-hdc` frames them: ADTS) into
DIR/station<k>_<offset in Hz>_p<program>.aac and prints one `program ... packets N bytes B` line per file at the end.
--dump-analog DIR writes every station's analog FM programme, demodulated on the device (nrsc5hip_fm_*), as DIR/station<k>_<offset in Hz>_analog.wav
(44.1 kHz, 16 bit, stereo; --deemphasis 75, 50 or 0 us) and prints one `analog frames N` line per file at the end.
--rds decodes RDS / RBDS of every station's analog host on the device and prints one line per report: `station 1 (+0.0 kHz): RDS PI 0x3AAB (KQED)`,
`... RDS PS "KEXP-FM "`, `... RDS RT "..."`, `... RDS clock MJD 60310 13:37 UTC-07:00`.
--eas watches every station's analog audio for Emergency Alert System bursts (SAME) on the device and prints one line per message:
`station 1 (+0.0 kHz): EAS WXR TOR 029095,029097 +0030 day 123 14:05 KXYZ/FM`, `... EAS end of message`.
--steer steers the analog audio by the reception of its own block -- stereo blend, high-cut, soft mute; --blend-db / --highcut-db / --mute-db LO,HI
set the CNR thresholds and imply it -- and prints `station 1 (+0.0 kHz): reception blend 0.42 high-cut 1.00 mute 1.00`.
--impair looks for the two impairments the CNR cannot tell apart and prints `station 1 (+0.0 kHz): reception multipath depth 0.30 (explained 0.88);
adjacent upper rho +0.91 usn -42.5 dB`, or `reception clear`, with a station's first audio and whenever a verdict changes.
--carrier measures every station's analog carrier on the device and prints `station 1 (+0.0 kHz): carrier -21.3 dBFS CNR 31.2 dB offset +0.41 kHz`
whenever the CNR has moved by 1 dB; --scan-analog makes the scan find analog-only FM stations as well (the spectrum nominates carriers, a measurement
of each one's CNR and centre error confirms them) and receives both kinds: `found +400.3 kHz analog score 18.8 dB carrier -54.7 dBFS CNR 15.3 dB ...`.
--dump-aas-files DIR writes every station's complete LOT files (album art, station logos, text files) as `nrsc5 --dump-aas-files` names them,
DIR/station<k>_<offset in Hz>_<lot>_<name>, and prints the reference's `SIG Service:` / `Audio component:` / `Data component:` / `LOT file:` lines; the
Station Information Guide and the files are put together on the device (nrsc5hip_aas_feed), only complete files reach the host.  FILE may be `-` (standard input, read in
--chunk pieces until it ends; --offsets is then required): the session may be of any length, the receiver gives FIFO space back as it
goes (nrsc5hip_batch_trim).  Without --offsets the stations are found
first (scan(): the band scan nrsc5hip_scan_* nominates centres from the capture's power spectrum, a short decode confirms them):

    python -m nrsc5_amd.wideband FILE --format cs16 --rate 20000000 [--scan-only] [--spectrum band.csv]

prints one `found` line per station, then decodes the whole file at the centres found."""
from __future__ import annotations

import argparse
import sys
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from . import engine as eng


class WidebandReceiver:
    """rate: S/s (int, Fraction or float); fmt: "cu8" | "cs16" | "cf32"; offsets_hz: one station centre per entry, relative to the
    capture centre.  push() takes interleaved samples as a host numpy array or a torch tensor on the device; every push decodes what
    it completes, and each station's events (records_to_log's ordered log, frames included) accumulate in `logs[k]`.
    q15_capacity: 744 187.5 S/s samples each station's engine stream holds.  A session may be of any length: when the next push
    would not fit, push() first gives back what nothing can read again (Engine.batch_trim: everything in front of the read
    position and of every replay checkpoint of l2_feedback whose verdict is still open).  The least capacity is
    eng.TRIM_RETAIN_MAX (9 195 120: the depth of the decode pipeline, include/nrsc5hip.h) + the outputs of the largest push
    (chan.outputs_for); the default carries any session at pushes of up to ~7.5 M outputs per station.  max_retained: the
    largest span a trim has left in a station's FIFO so far; trims: how many pushes had to trim.
    programs=True: the receiver also delivers every station's audio programs -- the reference's NRSC5_EVENT_HDC packets, in its order --
    through an HdcConsumer of its own: after the drains of a push, one eng.feed_hdc_batch call (nrsc5hip_hdc_feed) over all stations'
    new records; packets[s] collects (program, flags, bytes) and on_packet(station, program, flags, data), if given, sees each one.
    metadata=True: the receiver also reassembles every station's program service data on the device (PsdConsumer: one eng.feed_psd_batch
    call per push over all stations' new records; only finished AAS packets reach the host).  Packets on the PSD ports (0x5100,
    0x5201..0x5207) that hold an ID3v2.3 tag become ("id3", {"program", "title", "artist", "album", "genre"}) events behind that station's
    record events of the push, and now_playing[s][program] keeps the last tag; every other packet is kept raw in aas[s] as (program, port,
    seq, data); on_aas(station, program, port, seq, data), if given, sees every packet, tags included.  With programs=True as well the frames are indexed twice per push, once by each consumer.
    sis=True: the receiver also decodes every station's station information service on the device (SisConsumer: one eng.feed_sis_batch call per push over
    all stations' new records; 16 bytes per record go up, only events come back).  Every state change the reference reports becomes an event
    (eng.SIS_KINDS: "station_id", "station_name", "station_slogan", "station_message", "station_location", "audio_service", "data_service", "alert",
    "leap_second", "local_time", "exciter", "importer"; fields as eng.sis_event_fields) behind that station's record (and id3) events of the push, and
    station_info[s] is the station's snapshot (SisConsumer.info: country, fcc, name, slogan, message, alert, location, services).
    data_services=True: the receiver also follows every station's data services on the device (AasConsumer with lot_files file slots per station,
    chained behind the PsdConsumer, which it implies: one eng.feed_aas_batch call per push in place of eng.feed_psd_batch).  The PSD-port packets go
    down the same ID3 path as with metadata=True (id3 events, now_playing and on_aas are the same); the Station Information Guide becomes a
    ("sig", services) event and services[s] keeps it; a LOT header becomes a ("lot_header", fields) event, a complete file a ("lot", fields) event
    (eng.aas_event_fields: port, lot, size, mime, name, expiry, data), files[s][(port, lot)] keeps the last one and on_file(station, fields), if
    given, sees each; stream and packet data become ("stream" / "packet", fields) events.  No other packet reaches the host: aas[s] stays empty and
    on_aas sees the PSD-port packets only, so the host holds what the files take however long a carousel repeats.
    analog=True: the receiver also demodulates every station's analog FM programme on the device (eng.FmDemod behind the channelizer's staged
    outputs, nrsc5hip_chan_feed_fm: the channelized samples never visit the host; deemphasis_us 75, 50 or 0).  audio[s] collects int16 arrays
    of shape (n, 2) -- 44.1 kS/s stereo frames L, R -- and on_audio(station, pcm), if given, sees each push's new block; stereo[s] and pilot[s]
    hold the flag and the pilot level of the last block, and an ("analog", {"stereo", "pilot"}) event behind that station's other events of the
    push says when the flag changes.  The demodulator looks 18 359 input samples ahead and has no flush: the last 25 ms of a session stay undelivered.
    rds=True: the receiver also decodes RDS / RBDS of every station's analog host on the device (FmDemod(rds=True); it creates the FmDemod if
    analog did not, and audio is not collected then).  Every report of the decoder becomes an ("rds", {"kind": "pi" / "ps" / "rt" / "clock", ...})
    event (fields as eng.rds_event_fields) behind that station's other events of the push, and rds_info[s] is the station's snapshot
    (FmDemod.rds_get: pi, pty, flags, ps, rt, clock, synced).  A timing window of 152 bits is decided 96 431 input samples after its first
    sample is complete; there is no flush.
    eas=True: the receiver also watches every station's analog audio for EAS alerts -- SAME headers and end-of-message bursts, demodulated, framed
    and voted on the device (FmDemod(same=True); it creates the FmDemod if nothing else did, and audio is not collected then).  Every message
    the three-burst vote produces becomes an ("eas", {"text", "kind": "header" / "eom", "fields": eng.same_fields or None, "bursts", "first",
    "last"}) event returned by the push, and eas[s] keeps the station's messages so far; the logs are those of a receiver without it.  A window of
    64 bits is decided 92 693 input samples after its first sample; there is no flush.
    carrier=True: the receiver also measures every station's analog carrier on the device (FmDemod(carrier=True); it creates the FmDemod if
    neither analog nor rds did).  carrier[s] is the station's snapshot after every push (FmDemod.carrier: the windowed and the running level_db,
    cnr_db, offset_hz and the sums behind them), and a ("carrier", {"level_db", "cnr_db", "offset_hz"}) event is returned by the push whenever the
    windowed cnr_db has moved by 1 dB or more; the logs are those of a receiver without the measurement.
    steer=True (or a dict of FmDemod.steer_enable's arguments: blend_db, highcut_db, mute_db, mute_floor_db, controls): the analog audio is steered by
    the reception of its own block -- stereo blend, high-cut and soft mute on the device (FmDemod(steer=...)); it implies analog=True.  steer[s] is
    the station's snapshot after every push (FmDemod.steer: q, blend, highcut, mute at the end of the last audio block), and a ("steer", {...})
    event is returned by the push with the station's first audio and whenever its blend crosses 0.5 or its mute crosses the midpoint of its range:
    rare by design.  The logs are those of a receiver without steering.
    impair=True (or a dict of FmDemod.impair_enable's thresholds: explained_min, depth_min, rho_min): the receiver also looks for the two impairments
    that spoil an FM programme and that the CNR cannot tell apart -- multipath and a neighbour on one side -- on the device (FmDemod(impair=...)); it
    implies analog=True.  impair[s] is the station's snapshot after every push (FmDemod.impair: the windowed and the running figures, verdicts and
    sums), and an ("impair", {"multipath", "adjacent", "side", "explained", "depth", "rho", "usn_db", ...}) event of the windowed report is returned by
    the push with the station's first audio and whenever a verdict bit changes.  The logs are those of a receiver without it."""

    def __init__(self, rate, fmt: str, offsets_hz, device: int = 0, gains=None, q15_capacity: int = 1 << 24, lib_path: str | None = None,
                 programs: bool = False, on_packet=None, metadata: bool = False, on_aas=None, sis: bool = False, data_services: bool = False,
                 lot_files: int = 16, on_file=None, analog: bool = False, deemphasis_us: float = 75.0, on_audio=None, rds: bool = False,
                 carrier: bool = False, steer=False, eas: bool = False, impair=False):
        import torch
        self.fmt = eng.IQ_FORMATS[fmt]
        self.dtype = eng.IQ_DTYPES[self.fmt]
        self.dev = torch.device("cuda", device)
        self.offsets = [float(f) for f in offsets_hz]
        self.k = len(self.offsets)
        self.chan = eng.Channelizer(Fraction(rate) if not isinstance(rate, float) else rate, self.fmt, self.offsets, gains=gains,
                                    device=device, lib_path=lib_path)
        self.engine = eng.Engine(max_streams=self.k, q15_capacity=q15_capacity, record_capacity=512, p1_slots=16, p1_async=True,
                                 l2_feedback=True, device=device, lib_path=lib_path)
        self.ids = np.arange(self.k, dtype=np.int32)
        self.logs = [[] for _ in range(self.k)]
        self.records = [[] for _ in range(self.k)]
        self.q15_capacity = int(q15_capacity)
        self.held = 0                    # samples every station's FIFO holds (wr - base): the channelizer gives each station the same count
        self.max_retained = 0
        self.pushes = 0
        self.trims = 0
        self.programs = bool(programs)
        self.on_packet = on_packet
        self.packets = [[] for _ in range(self.k)]
        self.hdc = eng.HdcConsumer(self.k, lib=self.engine.lib) if self.programs else None
        self.metadata = bool(metadata)
        self.on_aas = on_aas
        self.data_services = bool(data_services)
        self.on_file = on_file
        self.psd = eng.PsdConsumer(self.engine, self.k) if self.metadata or self.data_services else None
        self.data = eng.AasConsumer(self.engine, self.k, lot_files=lot_files) if self.data_services else None
        self.services = [[] for _ in range(self.k)]
        self.files = [{} for _ in range(self.k)]
        self.now_playing = [{} for _ in range(self.k)]
        self.aas = [[] for _ in range(self.k)]
        self.sis = eng.SisConsumer(self.engine, self.k) if sis else None
        self.steer_enabled = bool(steer)
        self.impair_enabled = bool(impair)
        self.analog = bool(analog) or self.steer_enabled or self.impair_enabled
        self.on_audio = on_audio
        self.rds = bool(rds)
        self.carrier_enabled = bool(carrier)
        self.eas_enabled = bool(eas)
        self.eas = [[] for _ in range(self.k)]
        self.fm = None
        if self.analog or self.rds or self.carrier_enabled or self.eas_enabled:
            self.fm = eng.FmDemod(self.k, deemphasis_us=deemphasis_us, device=device, lib_path=lib_path, **({"rds": True} if self.rds else {}),
                                  **({"same": True, "same_burst_events": False} if self.eas_enabled else {}),
                                  **({"carrier": True} if self.carrier_enabled else {}), **({"steer": steer} if self.steer_enabled else {}),
                                  **({"impair": impair} if self.impair_enabled else {}))
        self.impair = [None] * self.k
        self._impair_said = [None] * self.k
        self.steer = [None] * self.k
        self._steer_side = [None] * self.k
        self.carrier = [None] * self.k
        self._carrier_said = [None] * self.k
        self.audio = [[] for _ in range(self.k)]
        self._audio_seen = False             # (the CLI clears audio[s] after every push)
        self.stereo = [False] * self.k
        self.pilot = [0.0] * self.k

    @property
    def station_info(self) -> list:
        """per station, the SIS snapshot (None without sis=True)"""
        return [None if self.sis is None else self.sis.info(s) for s in range(self.k)]

    @property
    def rds_info(self) -> list:
        """per station, the RDS snapshot (None without rds=True)"""
        return [self.fm.rds_get(s) if self.rds else None for s in range(self.k)]

    def _feed_sis(self, fresh, events):
        """fresh[s], events[s]: as for _feed_metadata"""
        if not any(len(r) for r in fresh):
            return
        for s, _, kind, v in eng.feed_sis_batch(self.sis, self.ids, fresh):
            self.logs[s].append((kind, v))
            events[s].append((s, kind, v))
        self.sis.events.clear()
        self.sis.raw.clear()

    def _packet(self, s, program, port, seq, data, events, keep: bool):
        """an AAS packet on the host: a tag of a PSD port becomes an id3 event; keep: anything else goes to aas[s]"""
        if self.on_aas is not None:
            self.on_aas(s, program, port, seq, data)
        tag = parse_id3(data) if is_psd_port(port) else None
        if tag is None:
            if keep:
                self.aas[s].append((program, port, seq, data))
            return
        v = {"program": port & 7, **tag}                            # output.c:881: the port names the program
        self.now_playing[s][port & 7] = tag
        self.logs[s].append(("id3", v))
        events[s].append((s, "id3", v))

    def _feed_metadata(self, fresh, events):
        """fresh[s]: as for _feed_programs; events[s]: the station's events of this push, which the id3 events go behind"""
        if not any(len(r) for r in fresh):
            return
        for s, program, port, seq, data in eng.feed_psd_batch(self.engine, self.psd, self.ids, fresh):
            self._packet(s, program, port, seq, data, events, True)
        self.psd.packets.clear()

    def _feed_data_services(self, fresh, events):
        """as _feed_metadata, with the data services chained behind the PSD transport on the device"""
        if not any(len(r) for r in fresh):
            return
        for s, kind, f in eng.feed_aas_batch(self.engine, self.data, self.psd, self.ids, fresh):
            if kind == "psd":
                self._packet(s, f["program"], f["port"], f["seq"], f["data"], events, False)
                continue
            if kind == "sig":
                self.services[s] = f
            elif kind == "lot":
                self.files[s][(f["port"], f["lot"])] = f
                if self.on_file is not None:
                    self.on_file(s, f)
            self.logs[s].append((kind, f))
            events[s].append((s, kind, f))
        self.data.events.clear()
        self.data.raw.clear()

    def _feed_programs(self, fresh):
        """fresh[s]: the records station s delivered in this push; their frames are still in the rings (nothing was processed since)"""
        if not any(len(r) for r in fresh):
            return
        self.hdc.events.clear()
        eng.feed_hdc_batch(self.engine, self.hdc, self.ids, fresh)
        for s, program, count, flags, data in self.hdc.events:
            self.packets[s].append((program, flags, data))
            if self.on_packet is not None:
                self.on_packet(s, program, flags, data)
        self.hdc.events.clear()

    def push(self, chunk) -> list:
        """-> the events this push produced: [(station, kind, fields), ...] in stream order per station"""
        import torch
        if isinstance(chunk, np.ndarray):
            chunk = torch.from_numpy(np.ascontiguousarray(chunk, dtype=self.dtype)).to(self.dev)
        chunk = chunk.contiguous()
        torch.cuda.current_stream(chunk.device).synchronize()      # the channelizer works on its own stream
        n = chunk.numel() // 2
        m = self.chan.outputs_for(n)
        if self.held + m > self.q15_capacity:                      # amortised: most pushes fit and copy nothing
            kept = self.engine.batch_trim(self.k, stream_ids=self.ids)
            self.held = int(kept.max())
            self.max_retained = max(self.max_retained, self.held)
            self.trims += 1
        pcm = None
        if self.fm is not None:
            cap = max(self.fm.outputs_for(m), 1)
            pcm = torch.empty((self.k, cap, 2), dtype=torch.int16, device=chunk.device)
            got = self.chan.feed_fm(self.engine, self.ids, self.fm, chunk.data_ptr(), n, pcm.data_ptr(), 2 * cap, cap)
            pcm = pcm[:, :got].cpu().numpy()
        else:
            self.chan.feed(self.engine, self.ids, chunk.data_ptr(), n)     # (still too large: EOVERFLOW from the append, nothing was touched)
        self.held += m
        self.pushes += 1
        self.engine.batch_process(self.k, stream_ids=self.ids)
        new = [[] for _ in range(self.k)]
        fresh = [None] * self.k
        for s in range(self.k):
            recs = self.engine.drain(s)
            fresh[s] = recs
            if len(recs):
                log = eng.records_to_log(self.engine, s, recs)          # frames are fetched now, while their ring slots hold them
                self.logs[s] += log
                self.records[s].append(recs)
                new[s] += [(s, kind, v) for kind, v in log]
        if self.programs:
            self._feed_programs(fresh)
        if self.data_services:
            self._feed_data_services(fresh, new)
        elif self.metadata:
            self._feed_metadata(fresh, new)
        if self.sis is not None:
            self._feed_sis(fresh, new)
        if self.analog:
            self._deliver_audio(pcm, new)
        if self.rds:
            for e in self.fm.rds_read():
                v = {"kind": e["kind"], **eng.rds_event_fields(e["kind"], e["v"], e["data"])}
                self.logs[e["channel"]].append(("rds", v))
                new[e["channel"]].append((e["channel"], "rds", v))
        if self.eas_enabled:
            for e in self.fm.same_read():                               # messages only: the bursts stay on the device
                v = {**eng.same_event_fields(e["kind"], e["v"], e["data"]), "first": e["first"], "last": e["last"]}
                self.eas[e["channel"]].append(v)
                new[e["channel"]].append((e["channel"], "eas", v))
        if self.carrier_enabled:
            self._measure_carrier(new)
        if self.steer_enabled:
            self._measure_steer(new)
        if self.impair_enabled:
            self._measure_impair(new)
        return [ev for per in new for ev in per]

    def _measure_impair(self, events):
        """impair[s]: the snapshot after this push; an ("impair", {...}) event of the windowed report with the first audio and whenever a verdict bit
        (multipath, adjacent, side) differs from the last one said (an event of the push only, as "carrier" is)"""
        self.impair = self.fm.impair()
        if not self._audio_seen:
            return
        for s, snap in enumerate(self.impair):
            w = snap["windowed"]
            said = (w["multipath"], w["adjacent"], w["side"])
            if said != self._impair_said[s]:
                self._impair_said[s] = said
                events[s].append((s, "impair", {k: w[k] for k in ("multipath", "adjacent", "side") + eng.FM_IMPAIR_FIGURES}))

    def _measure_steer(self, events):
        """steer[s]: the snapshot after this push; a ("steer", {...}) event with the first audio and whenever the blend has crossed 0.5 or the mute
        the midpoint of its range since the last one (an event of the push only, as "carrier" is)"""
        self.steer = self.fm.steer()
        if not self._audio_seen:
            return
        mid = 0.5 * (1.0 + 10.0 ** (self.fm.steer_config["mute_floor_db"] / 20.0))
        for s, snap in enumerate(self.steer):
            side = (snap["blend"] >= 0.5, snap["mute"] >= mid)
            if side != self._steer_side[s]:
                self._steer_side[s] = side
                events[s].append((s, "steer", dict(snap)))

    def _measure_carrier(self, events):
        """carrier[s]: the snapshot after this push; a ("carrier", {...}) event whenever the windowed cnr_db has moved by 1 dB or more since the
        last one (an event of the push only: the station's log is that of a receiver without the measurement)"""
        self.carrier = self.fm.carrier()
        for s, snap in enumerate(self.carrier):
            w = snap["windowed"]
            if snap["audio_blocks"] and (self._carrier_said[s] is None or abs(w["cnr_db"] - self._carrier_said[s]) >= 1.0):
                self._carrier_said[s] = w["cnr_db"]
                events[s].append((s, "carrier", {"level_db": w["level_db"], "cnr_db": w["cnr_db"], "offset_hz": w["offset_hz"]}))

    def _deliver_audio(self, pcm, events):
        """pcm: int16 [k, frames, 2], this push's new frames; events[s]: as for _feed_metadata"""
        if pcm.shape[1] == 0:
            return
        self._audio_seen = True
        level, flag = self.fm.pilot()
        for s in range(self.k):
            block = np.ascontiguousarray(pcm[s])
            self.audio[s].append(block)
            if self.on_audio is not None:
                self.on_audio(s, block)
            self.pilot[s] = float(level[s])
            if bool(flag[s]) != self.stereo[s]:
                self.stereo[s] = bool(flag[s])
                v = {"stereo": self.stereo[s], "pilot": self.pilot[s]}
                self.logs[s].append(("analog", v))
                events[s].append((s, "analog", v))

    def station_records(self, s: int) -> np.ndarray:
        return np.concatenate(self.records[s]) if self.records[s] else np.zeros(0, dtype=eng.RECORD_DTYPE)

    def close(self):
        if self.hdc is not None:
            self.hdc.close()
        if self.data is not None:
            self.data.close()
        if self.psd is not None:
            self.psd.close()
        if self.sis is not None:
            self.sis.close()
        if self.fm is not None:
            self.fm.close()
        self.engine.close()
        self.chan.close()


def is_psd_port(port: int) -> bool:
    """the AAS ports that carry a program's ID3 tags (output.c:878)"""
    return port == 0x5100 or 0x5201 <= port <= 0x5207


_ID3_TEXT = {b"TIT2": "title", b"TPE1": "artist", b"TALB": "album", b"TCON": "genre"}


def parse_id3(data: bytes) -> dict | None:
    """The text frames TIT2 / TPE1 / TALB / TCON of an ID3v2.3 tag as output_id3 reads them (output.c:277-322): None unless the tag starts
    "ID3" 3 0, flags 0, and its (sync-safe) length fits the data; the walk stops at a frame that runs over the tag.  Encoding 0 is Latin-1,
    1 is UTF-16 with a byte-order mark, anything else gives ""; a text ends at its first NUL.  -> {"title", "artist", "album", "genre"},
    each only if the tag holds it."""
    data = bytes(data)
    if len(data) < 10 or data[:5] != b"ID3\x03\x00" or data[5]:
        return None
    end = (((data[6] & 0x7f) << 21) | ((data[7] & 0x7f) << 14) | ((data[8] & 0x7f) << 7) | (data[9] & 0x7f)) + 10
    if end > len(data):
        return None
    out, off = {}, 10
    while off + 10 <= end:
        n = int.from_bytes(data[off + 4:off + 8], "big")
        if off + 10 + n > end:
            break
        key = _ID3_TEXT.get(data[off:off + 4])
        if key is not None:
            body = data[off + 10:off + 10 + n]
            if n == 0 or body[0] > 1:
                text = ""
            elif body[0] == 0:
                text = body[1:].decode("latin-1")
            else:
                text = body[1:len(body) - (len(body) - 1) % 2].decode("utf-16", errors="replace")
            out[key] = text.split("\0", 1)[0]
        off += 10 + n
    return out


CONFIRM_SECONDS = 1.0       # twice the largest first-PIDS time measured on the synthetic scenes, and not below 1 s
CONFIRM_MAX = 64            # nominations decoded by one confirmation pass, highest score first
NAME_SECONDS = 9.3          # scan(names=True): twice the largest first-name time measured on the synthetic scenes, 4.65 s


@dataclass
class FoundStation:
    offset_hz: float                     # centre relative to the capture centre (a bin centre of the survey)
    score_db: float
    lower_db: float
    upper_db: float
    floor_db: float = 0.0
    freq_offset_hz: float | None = None  # confirmed stations: what the engine's SYNC reports at that centre
    psmi: int | None = None
    pids_ok: int | None = None           # PIDS frames with a good CRC-12 inside the confirmation window
    first_pids_s: float | None = None    # capture time at the end of the push that delivered the first of them
    name: str | None = None              # scan(names=True): the station's name (SIS short or universal short name), e.g. "WXYZ-FM"
    country: str | None = None           # ... its country code and FCC facility id (SIS station id)
    facility_id: int | None = None
    first_name_s: float | None = None    # capture time at the end of the push that delivered the name
    kind: str = "hd"                     # "hd": a station that decodes; "analog": scan(analog=True) found a carrier without one
    cnr_db: float | None = None          # scan(analog=True): the running figures of the carrier measurement at offset_hz (cnr_db at the lower
    level_db: float | None = None        # ... clamp: no analog carrier there, e.g. an all-digital station)
    carrier_offset_hz: float | None = None   # ... the carrier sits at offset_hz + carrier_offset_hz
    stereo: bool | None = None           # ... the pilot flag and level of the last audio block
    pilot: float | None = None
    multipath: bool | None = None        # ... the two reception verdicts and their figures (FmDemod.impair), of the last audio block's window
    adjacent: bool | None = None
    adjacent_side: int | None = None     # +1: the neighbour is above, -1: below, 0: none
    explained: float | None = None
    depth: float | None = None
    rho: float | None = None
    usn_db: float | None = None


def _device_samples(raw, fmt: int, device: int):
    import torch
    dtype = eng.IQ_DTYPES[fmt]
    if isinstance(raw, np.ndarray):
        raw = torch.from_numpy(np.ascontiguousarray(raw, dtype=dtype)).to(torch.device("cuda", device))
    return raw.contiguous()


def survey(raw, rate, fmt: str, *, seconds: float | None = None, nfft: int = 0, threshold_db: float = 6.0, device: int = 0,
           lib_path: str | None = None):
    """power spectrum of the first `seconds` of the capture (all of it when None) and the detector's nominations
    -> (freqs_hz, psd, [FoundStation, ...] by ascending offset)"""
    code = eng.IQ_FORMATS[fmt]
    x = _device_samples(raw, code, device)
    n = x.numel() // 2
    if seconds is not None:
        n = min(n, int(seconds * float(Fraction(rate) if not isinstance(rate, float) else rate)))
    sc = eng.Scanner(Fraction(rate) if not isinstance(rate, float) else rate, code, nfft=nfft, device=device, lib_path=lib_path)
    try:
        sc.push_tensor(x[:2 * n])
        freqs, psd = sc.spectrum()
        picks = sc.detect(threshold_db=threshold_db)
    finally:
        sc.close()
    found = [FoundStation(p["offset_hz"], p["score_db"], p["lower_db"], p["upper_db"], p["floor_db"]) for p in picks]
    return freqs, psd, sorted(found, key=lambda s: s.offset_hz)


def confirm_stations(raw, rate, fmt: str, found, *, confirm_seconds: float = CONFIRM_SECONDS, chunk: int = 1 << 22, device: int = 0,
                     lib_path: str | None = None, names: bool = False, name_seconds: float | None = None) -> list:
    """decode the nominated centres (the CONFIRM_MAX best scores) over the first confirm_seconds of the capture in one engine; keep
    those whose stream reaches fine sync and delivers at least one PIDS frame with a good CRC-12.  names=True: the decode runs a SisConsumer
    and goes on behind the confirmation window, up to name_seconds (default NAME_SECONDS) of the capture, until every kept station has a name;
    name, country and facility_id of the stations are filled in from their SIS snapshots (None where none arrived in time)."""
    cands = sorted(found, key=lambda s: -s.score_db)[:CONFIRM_MAX]
    if not cands:
        return []
    fs = float(Fraction(rate) if not isinstance(rate, float) else rate)
    code = eng.IQ_FORMATS[fmt]
    x = _device_samples(raw, code, device)
    n = min(x.numel() // 2, int(confirm_seconds * fs))
    n_names = max(n, min(x.numel() // 2, int((NAME_SECONDS if name_seconds is None else name_seconds) * fs))) if names else n
    q15 = int(n_names / fs * 744187.5) + 4 * 71280
    rx = WidebandReceiver(rate, fmt, [s.offset_hz for s in cands], device=device, q15_capacity=q15, lib_path=lib_path, sis=names)

    def push(p, limit):
        end = min(limit, p + chunk)
        rx.push(x[2 * p:2 * end])
        for k, s in enumerate(cands):
            if s.first_pids_s is None and rx.records[k]:
                fl = rx.records[k][-1]["flags"]
                if np.any(((fl & eng.REC_PIDS) != 0) & ((fl & eng.REC_PIDS_CRC) != 0)):
                    s.first_pids_s = end / fs
            if names and s.name is None:
                info = rx.sis.info(k)
                if info["name"] is not None:
                    s.name, s.first_name_s = info["name"], end / fs
        return end
    try:
        for p in range(0, n, chunk):
            push(p, n)
        kept = []
        for k, s in enumerate(cands):
            recs = rx.station_records(k)
            fl = recs["flags"]
            fine = np.nonzero(fl & eng.REC_TO_FINE)[0]
            good = int(np.sum(((fl & eng.REC_PIDS) != 0) & ((fl & eng.REC_PIDS_CRC) != 0)))
            if fine.size and good:
                s.freq_offset_hz, s.psmi, s.pids_ok = float(recs["freq_offset"][fine[0]]), int(recs["psmi"][fine[0]]), good
                kept.append(s)
        p = n
        while names and p < n_names and any(s.name is None for s in kept):
            p = push(p, n_names)
        if names:
            for k, s in enumerate(cands):
                info = rx.sis.info(k)
                s.country, s.facility_id = info["country"], (info["fcc"] if info["fcc"] >= 0 else None)
    finally:
        rx.close()
    return sorted(kept, key=lambda s: s.offset_hz)


MIN_CNR_DB = 10.0           # confirm_analog: the FM threshold
MAX_OFFSET_HZ = 5e3         # ... transmitters hold +-2 kHz, and a 20 ppm SDR adds 2 kHz at 100 MHz
HD_GUARD_HZ = 100e3         # scan(analog=True): an analog nomination this close to a confirmed HD station is that station's host or sideband


def survey_fm(raw, rate, fmt: str, *, seconds: float | None = None, nfft: int = 0, threshold_db: float = 6.0, device: int = 0,
              lib_path: str | None = None) -> list:
    """the analog-carrier detector's nominations over the first `seconds` of the capture -> [FoundStation(kind="analog"), ...] by ascending offset"""
    code = eng.IQ_FORMATS[fmt]
    x = _device_samples(raw, code, device)
    n = x.numel() // 2
    if seconds is not None:
        n = min(n, int(seconds * float(Fraction(rate) if not isinstance(rate, float) else rate)))
    sc = eng.Scanner(Fraction(rate) if not isinstance(rate, float) else rate, code, nfft=nfft, device=device, lib_path=lib_path)
    try:
        sc.push_tensor(x[:2 * n])
        picks = sc.detect_fm(threshold_db=threshold_db)
    finally:
        sc.close()
    return sorted((FoundStation(p["offset_hz"], p["score_db"], 0.0, 0.0, p["floor_db"], kind="analog") for p in picks), key=lambda s: s.offset_hz)


def measure_carriers(x, n: int, rate, code: int, centres, *, chunk: int = 1 << 22, device: int = 0, lib_path: str | None = None, rds: bool = False,
                     seconds_rds: float | None = None, impair: bool = False):
    """the first n samples of the device tensor x through a Channelizer at `centres` and an FmDemod(carrier=True) behind it, no engine
    -> (FmDemod.carrier() snapshots, pilot levels, stereo flags, rds snapshots or None); impair=True: the same pass also runs the impairment
    detectors, and every carrier snapshot carries FmDemod.impair()'s under the key "impair" """
    import torch
    ch = eng.Channelizer(rate, code, centres, device=device, lib_path=lib_path)
    fm = eng.FmDemod(len(centres), device=device, lib_path=lib_path, carrier=True, rds=rds, impair=impair)
    try:
        for p in range(0, n, chunk):
            y = ch.process_tensor(x[2 * p:2 * min(n, p + chunk)])
            if y.shape[1]:
                fm.process_tensor(y)
        level, flag = fm.pilot()
        snaps = fm.carrier()
        if impair:
            for snap, v in zip(snaps, fm.impair()):
                snap["impair"] = v
        return snaps, level, flag, ([fm.rds_get(k) for k in range(len(centres))] if rds else None)
    finally:
        fm.close()
        ch.close()


def confirm_analog(raw, rate, fmt: str, found, *, confirm_seconds: float = CONFIRM_SECONDS, min_cnr_db: float = MIN_CNR_DB,
                   max_offset_hz: float = MAX_OFFSET_HZ, chunk: int = 1 << 22, device: int = 0, lib_path: str | None = None, names: bool = False,
                   name_seconds: float | None = None, keep_all: bool = False) -> list:
    """measure the carriers of the nominated centres (the CONFIRM_MAX best scores) over the first confirm_seconds of the capture, twice: at the
    nominated centres, then at the centres corrected by the running offset_hz of the first pass.  Kept: second-pass running cnr_db >= min_cnr_db
    and |offset_hz| <= max_offset_hz; a kept station's offset_hz is the corrected centre.  keep_all=True returns every candidate with its
    figures (the hosts of HD stations: scan(analog=True)), uncorrected.  names=True: the second pass also decodes RDS, over name_seconds
    (default NAME_SECONDS), and name is rds_callsign(PI) or else the PS."""
    cands = sorted(found, key=lambda s: -s.score_db)[:CONFIRM_MAX]
    if not cands:
        return []
    rate = Fraction(rate) if not isinstance(rate, float) else rate
    fs = float(rate)
    code = eng.IQ_FORMATS[fmt]
    x = _device_samples(raw, code, device)
    n = min(x.numel() // 2, int(confirm_seconds * fs))
    centres = [s.offset_hz for s in cands]
    if not keep_all:
        first, _, _, _ = measure_carriers(x, n, rate, code, centres, chunk=chunk, device=device, lib_path=lib_path)
        centres = [c + v["running"]["offset_hz"] for c, v in zip(centres, first)]
    n2 = max(n, min(x.numel() // 2, int((NAME_SECONDS if name_seconds is None else name_seconds) * fs))) if names else n
    snaps, level, flag, rds = measure_carriers(x, n2, rate, code, centres, chunk=chunk, device=device, lib_path=lib_path, rds=names, impair=True)
    kept = []
    for k, s in enumerate(cands):
        r = snaps[k]["running"]
        s.offset_hz = centres[k]
        s.cnr_db, s.level_db, s.carrier_offset_hz, s.stereo, s.pilot = r["cnr_db"], r["level_db"], r["offset_hz"], bool(flag[k]), float(level[k])
        w = snaps[k]["impair"]["windowed"]
        s.multipath, s.adjacent, s.adjacent_side = w["multipath"], w["adjacent"], w["side"]
        s.explained, s.depth, s.rho, s.usn_db = w["explained"], w["depth"], w["rho"], w["usn_db"]
        if names and s.name is None and rds[k]["pi"] >= 0:
            s.name = eng.rds_callsign(rds[k]["pi"]) or (rds[k]["ps"].decode("latin-1").strip() if rds[k]["ps"] else None)
        if keep_all or (r["cnr_db"] >= min_cnr_db and abs(r["offset_hz"]) <= max_offset_hz):
            kept.append(s)
    return sorted(kept, key=lambda s: s.offset_hz)


def scan(raw, rate, fmt: str, *, seconds: float | None = None, confirm: bool = True, confirm_seconds: float = CONFIRM_SECONDS,
         threshold_db: float = 6.0, device: int = 0, lib_path: str | None = None, names: bool = False, name_seconds: float | None = None,
         analog: bool = False, min_cnr_db: float = MIN_CNR_DB, max_offset_hz: float = MAX_OFFSET_HZ) -> list:
    """Find the HD stations of a capture.  raw: interleaved samples (numpy array, or torch tensor on the device) in `fmt` at `rate` S/s.
    The spectrum is taken over the first `seconds` (None: everything); confirm=False returns the detector's nominations, confirm=True
    only those that decode (fine sync and a PIDS frame with a good CRC) within the first confirm_seconds.  names=True: the confirmation decode
    also reads the stations' SIS and keeps decoding a confirmed station until its name arrived, up to name_seconds (default NAME_SECONDS) of the
    capture: FoundStation.name / country / facility_id.  analog=True: analog-only FM stations are found as well (scan_analog: kind "analog", their
    name from RDS with names=True), and the HD stations carry the figures of their hosts' carriers.  -> [FoundStation, ...] by ascending offset."""
    _, _, found = survey(raw, rate, fmt, seconds=seconds, threshold_db=threshold_db, device=device, lib_path=lib_path)
    if not confirm:
        return found
    hd = confirm_stations(raw, rate, fmt, found, confirm_seconds=confirm_seconds, device=device, lib_path=lib_path, names=names, name_seconds=name_seconds)
    if not analog:
        return hd
    return scan_analog(raw, rate, fmt, hd, seconds=seconds, confirm_seconds=confirm_seconds, threshold_db=threshold_db, device=device, lib_path=lib_path,
                       names=names, name_seconds=name_seconds, min_cnr_db=min_cnr_db, max_offset_hz=max_offset_hz)


def scan_analog(raw, rate, fmt: str, hd, *, seconds: float | None = None, confirm_seconds: float = CONFIRM_SECONDS, threshold_db: float = 6.0,
                device: int = 0, lib_path: str | None = None, names: bool = False, name_seconds: float | None = None,
                min_cnr_db: float = MIN_CNR_DB, max_offset_hz: float = MAX_OFFSET_HZ) -> list:
    """the analog half of scan(analog=True): hd (the confirmed HD stations) gain the figures of their hosts, and every kept analog nomination
    that is not within HD_GUARD_HZ of one of them -- its host, or one of its sidebands -- joins them.  -> [FoundStation, ...] by ascending offset"""
    nominated = survey_fm(raw, rate, fmt, seconds=seconds, threshold_db=threshold_db, device=device, lib_path=lib_path)
    kept = confirm_analog(raw, rate, fmt, nominated, confirm_seconds=confirm_seconds, min_cnr_db=min_cnr_db, max_offset_hz=max_offset_hz, device=device,
                          lib_path=lib_path, names=names, name_seconds=name_seconds)
    kept = [s for s in kept if all(abs(s.offset_hz - h.offset_hz) > HD_GUARD_HZ for h in hd)]
    confirm_analog(raw, rate, fmt, hd, confirm_seconds=confirm_seconds, device=device, lib_path=lib_path, keep_all=True)
    return sorted(list(hd) + kept, key=lambda s: s.offset_hz)


def format_found(s: FoundStation) -> str:
    line = f"found {s.offset_hz / 1e3:+.1f} kHz score {s.score_db:.1f} dB lower {s.lower_db:.1f} upper {s.upper_db:.1f}"
    if s.kind == "analog":
        line = f"found {s.offset_hz / 1e3:+.1f} kHz analog score {s.score_db:.1f} dB"
    line += f" psmi {s.psmi}" if s.psmi is not None else ""
    if s.cnr_db is not None:
        line += f" carrier {s.level_db:.1f} dBFS CNR {s.cnr_db:.1f} dB offset {s.carrier_offset_hz / 1e3:+.2f} kHz {'stereo' if s.stereo else 'mono'}"
    if s.multipath or s.adjacent:
        line += " reception " + _impair_words(dict(multipath=s.multipath, adjacent=s.adjacent, side=s.adjacent_side, explained=s.explained, depth=s.depth,
                                                   rho=s.rho, usn_db=s.usn_db))
    return line + (f" name {s.name}" if s.name is not None else "")


def write_spectrum_csv(path: str, freqs, psd):
    with open(path, "w") as f:
        f.write("freq_hz,power_db\n")
        for fr, p in zip(freqs, psd):
            f.write(f"{fr:.3f},{10 * np.log10(max(p, 1e-30)):.3f}\n")


def _impair_words(v: dict) -> str:
    """`multipath depth 0.30 (explained 0.88); adjacent upper rho +0.91 usn -42.5 dB`, or `clear`"""
    words = []
    if v["multipath"]:
        words.append(f"multipath depth {v['depth']:.2f} (explained {v['explained']:.2f})")
    if v["adjacent"]:
        words.append(f"adjacent {'upper' if v['side'] > 0 else 'lower'} rho {v['rho']:+.2f} usn {v['usn_db']:.1f} dB")
    return "; ".join(words) or "clear"


def format_event(rx: WidebandReceiver, s: int, kind: str, v: dict) -> str | None:
    head = f"station {s} ({rx.offsets[s] / 1e3:+.1f} kHz):"
    if kind == "sync":
        return f"{head} SYNC freq_offset={v['freq_offset']:.1f} Hz psmi={v['psmi']}"
    if kind == "mer":
        return f"{head} MER lower={v['lower']:.1f} dB upper={v['upper']:.1f} dB"
    if kind == "ber":
        return f"{head} BER {v['cber']:.6f}"
    if kind == "lost_sync":
        return f"{head} LOST_SYNC"
    if kind == "id3":
        return f"{head} ID3 program {v['program']}" + "".join(f" {k}={v[k]!r}" for k in ("title", "artist", "album", "genre") if k in v)
    if kind in _SIS_LINES:
        return f"{head} " + _SIS_LINES[kind](v)
    if kind == "carrier":
        return f"{head} carrier {v['level_db']:.1f} dBFS CNR {v['cnr_db']:.1f} dB offset {v['offset_hz'] / 1e3:+.2f} kHz"
    if kind == "steer":
        return f"{head} reception blend {v['blend']:.2f} high-cut {v['highcut']:.2f} mute {v['mute']:.2f}"
    if kind == "impair":
        return f"{head} reception " + _impair_words(v)
    if kind == "eas":
        return f"{head} " + eng.same_line(v["text"])
    if kind == "rds":
        if v["kind"] == "pi":
            return f"{head} RDS PI 0x{v['pi']:04X}" + (f" ({v['callsign']})" if v["callsign"] else "")
        if v["kind"] == "ps":
            return f"{head} RDS PS \"{v['raw'].decode('latin-1')}\""
        if v["kind"] == "rt":
            return f"{head} RDS RT \"{v['text']}\""
        if v["kind"] == "clock":
            off = v["offset_half_hours"]
            return f"{head} RDS clock MJD {v['mjd']} {v['hour']:02d}:{v['minute']:02d} UTC{'-' if off < 0 else '+'}{abs(off) // 2:02d}:{abs(off) % 2 * 30:02d}"
        return None
    if kind == "sig":                                               # main.c:416-438
        lines = []
        for sv in v:
            lines.append(f"{head} SIG Service: type={sv['type']} number={sv['number']} name={sv['name']}")
            for c in sv["components"]:
                if c["type"] == "audio":
                    lines.append(f"{head}   Audio component: id={c['id']} port={c['port']:04X} type={c['data_type']} mime={c['mime']:08X}")
                else:
                    lines.append(f"{head}   Data component: id={c['id']} port={c['port']:04X} service_data_type={c['service_data_type']} type={c['data_type']} mime={c['mime']:08X}")
        return "\n".join(lines) if lines else None
    if kind == "lot":                                               # main.c:445-450
        y, mo, d, h, mi = v["expiry"]
        return (f"{head} LOT file: port={v['port']:04X} lot={v['lot']} name={v['name']} size={v['size']} mime={v['mime']:08X} "
                f"expiry={y + 1900:04d}-{mo + 1:02d}-{d:02d}T{h:02d}:{mi:02d}:00Z")
    return None


def _device_line(what):
    return lambda v: (f"{what} {v['manufacturer_id']!r} core {'.'.join(map(str, v['core_version']))}-{v['core_status']} "
                      f"manufacturer {'.'.join(map(str, v['manufacturer_version']))}-{v['manufacturer_status']}"
                      + (f" importer_connected={v['importer_connected']}" if "importer_connected" in v else ""))


_SIS_LINES = {
    "station_id": lambda v: f"STATION_ID country={v['country']} facility_id={v['fcc']}",
    "station_name": lambda v: f"STATION_NAME {v['name']!r}",
    "station_slogan": lambda v: f"STATION_SLOGAN {v['slogan']!r}",
    "station_message": lambda v: f"STATION_MESSAGE {v['message']!r}",
    "station_location": lambda v: f"STATION_LOCATION latitude={v['latitude']:.4f} longitude={v['longitude']:.4f} altitude={v['altitude']} m",
    "audio_service": lambda v: f"AUDIO_SERVICE program={v['program']} access={v['access']} type={v['type']} sound_exp={v['sound_exp']}",
    "data_service": lambda v: f"DATA_SERVICE access={v['access']} type={v['type']} mime_type={v['mime_type']:03x}",
    "alert": lambda v: "ALERT ended" if v["control_data"] is None else f"ALERT {v['message']!r} control_data={v['control_data'].hex()}",
    "leap_second": lambda v: f"LEAP_SECOND pending_offset={v['pending_offset']} current_offset={v['current_offset']} pending_alfn={v['pending_alfn']}",
    "local_time": lambda v: f"LOCAL_TIME utc_offset={v['utc_offset']} min dst_regional={v['dst_regional']} dst_local={v['dst_local']} dst_schedule={v['dst_schedule']}",
    "exciter": _device_line("EXCITER"),
    "importer": _device_line("IMPORTER"),
}


class HdcDump:
    """--dump-hdc: one ADTS file per station and program, opened on the first packet that carries data.  A packet without data
    (one that failed its CRC) would be a 7-byte header with no frame behind it: it is left out of the file and of the counts.  adts: the framing function (HdcConsumer.adts: nrsc5hip_hdc_adts)."""

    def __init__(self, directory: str, offsets_hz, adts):
        import os
        os.makedirs(directory, exist_ok=True)
        self.dir, self.offsets, self.adts = directory, [float(f) for f in offsets_hz], adts
        self.files = {}                  # (station, program) -> [file, packets, bytes]

    def path(self, station: int, program: int) -> str:
        import os
        return os.path.join(self.dir, f"station{station}_{int(round(self.offsets[station])):+d}_p{program}.aac")

    def write(self, station: int, program: int, flags: int, data: bytes):
        if not data:
            return
        ent = self.files.get((station, program))
        if ent is None:
            ent = self.files[(station, program)] = [open(self.path(station, program), "wb"), 0, 0]
        frame = self.adts(data)
        ent[0].write(frame)
        ent[1] += 1
        ent[2] += len(frame)

    def flush(self):
        for ent in self.files.values():
            ent[0].flush()

    def close(self) -> list:
        """-> the summary lines, by station and program"""
        lines = []
        for (s, p), (f, n, nbytes) in sorted(self.files.items()):
            f.close()
            lines.append(f"station {s} ({self.offsets[s] / 1e3:+.1f} kHz): program {p} packets {n} bytes {nbytes}")
        return lines


class AasDump:
    """--dump-aas-files: every complete LOT file as the reference names it, <lot>_<name> (main.c:253), prefixed like --dump-hdc; path separators in the
    name are replaced"""

    def __init__(self, directory: str, offsets_hz):
        import os
        os.makedirs(directory, exist_ok=True)
        self.dir, self.offsets = directory, [float(f) for f in offsets_hz]

    def path(self, station: int, lot: int, name: str) -> str:
        import os
        safe = name.replace("/", "_").replace("\\", "_").replace("\0", "_")
        return os.path.join(self.dir, f"station{station}_{int(round(self.offsets[station])):+d}_{lot}_{safe}")

    def write(self, station: int, f: dict):
        with open(self.path(station, f["lot"], f["name"]), "wb") as out:
            out.write(f["data"])


class AnalogDump:
    """--dump-analog: one WAV file per station (44.1 kHz, 16 bit, stereo), opened on the station's first audio.  Every write leaves a
    complete file behind it -- the header is brought up to date and the file flushed -- so a live pipe does not hold its audio."""

    def __init__(self, directory: str, offsets_hz):
        import os
        os.makedirs(directory, exist_ok=True)
        self.dir, self.offsets = directory, [float(f) for f in offsets_hz]
        self.files = {}                  # station -> [file, wave writer, frames]

    def path(self, station: int) -> str:
        import os
        return os.path.join(self.dir, f"station{station}_{int(round(self.offsets[station])):+d}_analog.wav")

    def write(self, station: int, pcm):
        import wave
        if not len(pcm):
            return
        ent = self.files.get(station)
        if ent is None:
            f = open(self.path(station), "wb")
            w = wave.open(f, "wb")
            w.setnchannels(2); w.setsampwidth(2); w.setframerate(eng.FM_AUDIO_RATE)
            ent = self.files[station] = [f, w, 0]
        ent[1].writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())      # (writeframes patches the header's lengths)
        ent[0].flush()
        ent[2] += len(pcm)

    def close(self) -> list:
        """-> the summary lines, by station"""
        lines = []
        for s, (f, w, frames) in sorted(self.files.items()):
            w.close()
            f.close()
            lines.append(f"station {s} ({self.offsets[s] / 1e3:+.1f} kHz): analog frames {frames} seconds {frames / eng.FM_AUDIO_RATE:.3f}")
        return lines


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m nrsc5_amd.wideband", description=__doc__.splitlines()[0])
    ap.add_argument("file", help="capture file, or - for standard input (needs --offsets)")
    ap.add_argument("--format", choices=sorted(eng.IQ_FORMATS), default="cs16")
    ap.add_argument("--rate", required=True, help="S/s, an integer or a fraction num/den")
    ap.add_argument("--offsets", default=None, help="comma-separated station centres in Hz relative to the capture centre (default: --scan)")
    ap.add_argument("--scan", action="store_true", help="find the stations first and print them (implied without --offsets)")
    ap.add_argument("--scan-only", action="store_true", help="stop after the list of stations")
    ap.add_argument("--scan-seconds", type=float, default=CONFIRM_SECONDS, help="how much of the file the scan looks at")
    ap.add_argument("--threshold-db", type=float, default=6.0, help="least detector score of a nomination")
    ap.add_argument("--spectrum", metavar="FILE.csv", default=None, help="write the scan's power spectrum: freq_hz,power_db per bin")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=1 << 22, help="samples per push")
    ap.add_argument("--q15-capacity", type=int, default=1 << 24,
                    help="decimated samples of FIFO per station: at least %d + the outputs of one push, whatever the length of the session" % eng.TRIM_RETAIN_MAX)
    ap.add_argument("--dump-hdc", metavar="DIR", default=None,
                    help="write every station's audio programs as ADTS: DIR/station<k>_<offset in Hz>_p<program>.aac")
    ap.add_argument("--dump-aas-files", metavar="DIR", default=None,
                    help="write every station's complete LOT files (album art, logos): DIR/station<k>_<offset in Hz>_<lot>_<name>; prints the SIG and a line per file")
    ap.add_argument("--dump-analog", metavar="DIR", default=None,
                    help="write every station's analog FM programme as WAV (44.1 kHz, 16 bit, stereo): DIR/station<k>_<offset in Hz>_analog.wav")
    ap.add_argument("--deemphasis", type=float, default=75.0, choices=[75.0, 50.0, 0.0], help="de-emphasis of the analog audio in us (0: none)")
    ap.add_argument("--metadata", action="store_true", help="print what every program is playing (ID3 tags of the program service data)")
    ap.add_argument("--eas", action="store_true", help="print the EAS alerts (SAME headers and end of message) in every station's analog audio, one line per message")
    ap.add_argument("--rds", action="store_true", help="print RDS / RBDS of every station's analog host: PI (and the call sign it encodes), name, RadioText, clock")
    ap.add_argument("--carrier", action="store_true", help="print level, CNR and centre error of every station's analog carrier whenever the CNR has moved by 1 dB")
    ap.add_argument("--steer", action="store_true", help="steer the analog audio by reception: stereo blend, high-cut and soft mute (with --dump-analog); prints "
                    "`reception blend B high-cut H mute G` with a station's first audio and when its blend crosses 0.5 or its mute the midpoint of its range")
    pair = lambda t: tuple(float(v) for v in t.split(","))
    ap.add_argument("--blend-db", type=pair, metavar="LO,HI", default=None, help="CNR in dB where the stereo blend starts and where it is complete (18,30); implies --steer")
    ap.add_argument("--highcut-db", type=pair, metavar="LO,HI", default=None, help="CNR in dB where the high-cut is full and where it ends (10,20); implies --steer")
    ap.add_argument("--mute-db", type=pair, metavar="LO,HI", default=None, help="CNR in dB where the soft mute is at its floor and where it ends (2,8); implies --steer")
    ap.add_argument("--impair", action="store_true", help="look for multipath and for a neighbour on one side in every station's analog carrier: prints "
                    "`reception multipath depth D (explained E); adjacent upper rho R usn U dB` or `reception clear` with a station's first audio and when a verdict changes")
    ap.add_argument("--scan-analog", action="store_true", help="scan for analog-only FM stations as well as HD stations, and receive both")
    ap.add_argument("--sis", action="store_true", help="print who every station is: id, name, slogan, message, location, services, alerts; a scan then prints the call sign on every `found` line")
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):                  # "--offsets -800e3,0,400e3": a value that starts with '-' is still the value
        if argv[i] == "--offsets":
            argv[i:i + 2] = ["--offsets=" + argv[i + 1]]
            break
    for name in ("--blend-db", "--highcut-db", "--mute-db"):
        for i in range(len(argv) - 1):
            if argv[i] == name:
                argv[i:i + 2] = [name + "=" + argv[i + 1]]
                break
    a = ap.parse_args(argv)
    rate = Fraction(a.rate)
    offsets = None if a.offsets is None else [float(x) for x in a.offsets.split(",") if x]
    fmt = eng.IQ_FORMATS[a.format]
    dtype = eng.IQ_DTYPES[fmt]
    stdin = a.file == "-"
    do_scan = a.scan or a.scan_only or a.scan_analog or offsets is None
    if stdin and (do_scan or a.spectrum):
        ap.error("standard input cannot be scanned (the scan reads the head of a real file): give --offsets, without --scan / --spectrum")
    if do_scan or a.spectrum:
        head = np.fromfile(a.file, dtype=dtype, count=2 * int(max(a.scan_seconds, NAME_SECONDS if a.sis else 0.0) * float(rate)))
        head = _device_samples(head, fmt, a.device)
        freqs, psd, found = survey(head, rate, a.format, seconds=a.scan_seconds, threshold_db=a.threshold_db, device=a.device)
        if a.spectrum:
            write_spectrum_csv(a.spectrum, freqs, psd)
        if do_scan:
            found = confirm_stations(head, rate, a.format, found, confirm_seconds=a.scan_seconds, device=a.device, names=a.sis)
            if a.scan_analog:
                found = scan_analog(head, rate, a.format, found, seconds=a.scan_seconds, confirm_seconds=a.scan_seconds, threshold_db=a.threshold_db,
                                    device=a.device, names=a.rds)
            for s in found:
                print(format_found(s), flush=True)
            if a.scan_only:
                return 0
            if offsets is None:
                offsets = [s.offset_hz for s in found]
                if not offsets:
                    print("no station found", file=sys.stderr)
                    return 1
        del head
    steer = False
    if a.steer or a.blend_db or a.highcut_db or a.mute_db:
        steer = {k: v for k, v in (("blend_db", a.blend_db), ("highcut_db", a.highcut_db), ("mute_db", a.mute_db)) if v is not None} or True
        for v in (a.blend_db, a.highcut_db, a.mute_db):
            if v is not None and len(v) != 2:
                ap.error("a threshold pair is LO,HI")
    rx = WidebandReceiver(rate, a.format, offsets, device=a.device, q15_capacity=a.q15_capacity, programs=a.dump_hdc is not None, metadata=a.metadata, sis=a.sis,
                          data_services=a.dump_aas_files is not None, analog=a.dump_analog is not None, deemphasis_us=a.deemphasis, rds=a.rds,
                          carrier=a.carrier, steer=steer, eas=a.eas, impair=a.impair)
    wav = None
    if a.dump_analog is not None:
        wav = AnalogDump(a.dump_analog, offsets)
        rx.on_audio = wav.write
    if a.dump_aas_files is not None:
        rx.on_file = AasDump(a.dump_aas_files, offsets).write
    dump = None
    if a.dump_hdc is not None:
        dump = HdcDump(a.dump_hdc, offsets, rx.hdc.adts)
        rx.on_packet = dump.write
    item = 2 * np.dtype(dtype).itemsize
    with (sys.stdin.buffer if stdin else open(a.file, "rb")) as f:
        while True:
            raw = f.read(item * a.chunk)                       # (a pipe: read() returns short only at the end of the stream)
            buf = np.frombuffer(bytearray(raw[:len(raw) - len(raw) % item]), dtype=dtype)
            if buf.size < 2:
                break
            for s, kind, v in rx.push(buf[:buf.size - buf.size % 2]):
                line = format_event(rx, s, kind, v)
                if line:
                    print(line, flush=True)
            if wav is not None or steer or a.impair:
                for kept in rx.audio:                          # written and flushed by on_audio (or, steered without a dump, not wanted)
                    kept.clear()
            if dump is not None:
                dump.flush()
                for kept in rx.packets:                        # written: a session of any length must not keep its audio in memory
                    kept.clear()
    if dump is not None:
        for line in dump.close():
            print(line, flush=True)
    if wav is not None:
        for line in wav.close():
            print(line, flush=True)
    rx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
