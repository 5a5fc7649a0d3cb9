"""The PSD transport rules of include/nrsc5hip.h (nrsc5hip_psd_*) restated in plain Python, byte by byte -- the model the device code
(csrc/k_psd.hip) is compared with, as chan_model.py is for the channelizer.  It is itself pinned against the unmodified reference
(parse_hdlc / aas_push, frame.c:328-391) in tests/test_psd_stage_cpu.py: fed from the oracle's L2 index it gives the reference's
`l2aas` records frame by frame.

State per program: psd_buf / psd_idx of frame_t.  Input per frame: the L2 index as a dict (oracle.l2_index / eng.l2_frame_to_dict) and the
frame's PDU bytes."""
from __future__ import annotations

MAX_AAS_LEN = 8212                                   # frame.h:5
STATS = ("pdus", "span_bytes", "closed", "empty", "bad_fcs", "wrong_protocol", "truncated_escape", "overflows", "delivered")


def fcs16(data: bytes) -> int:
    crc = 0xFFFF
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    return crc


class PsdModel:
    def __init__(self):
        self.buf = [bytearray() for _ in range(8)]
        self.idx = [-1] * 8
        self.stats = dict.fromkeys(STATS, 0)

    def reset(self):
        """frame_reset: every program closed"""
        self.idx = [-1] * 8

    def _close(self, program: int, out: list):
        raw = bytes(self.buf[program][:self.idx[program]])
        st = self.stats
        st["closed"] += 1
        data = bytearray()
        i = 0
        while i < len(raw):
            if raw[i] == 0x7D:
                if i + 1 == len(raw):                # an unpaired escape at the end: dropped (the reference ORs a stale byte in)
                    st["truncated_escape"] += 1
                    return
                data.append(raw[i + 1] | 0x20)       # OR, frame.c:335
                i += 2
            else:
                data.append(raw[i])
                i += 1
        if not data:
            st["empty"] += 1
        elif fcs16(data) != 0xF0B8:
            st["bad_fcs"] += 1
        elif data[0] != 0x21 or len(data) < 7:       # shorter than protocol + port + seq + FCS: the reference reads past the packet
            st["wrong_protocol"] += 1
        else:
            pkt = bytes(data[1:-2])
            st["delivered"] += 1
            out.append((program, pkt[0] | pkt[1] << 8, pkt[2] | pkt[3] << 8, pkt[4:]))

    def push_bytes(self, program: int, span: bytes) -> list:
        out = []
        for b in span:
            if b == 0x7E:
                if self.idx[program] >= 0:
                    self._close(program, out)
                self.idx[program] = 0
            elif self.idx[program] >= 0:
                if self.idx[program] == MAX_AAS_LEN:
                    self.idx[program] = -1
                    self.stats["overflows"] += 1
                    continue
                k = self.idx[program]
                if k < len(self.buf[program]):
                    self.buf[program][k] = b
                else:
                    self.buf[program].append(b)
                self.idx[program] = k + 1
        return out

    def push_frame(self, index: dict, pdu_bytes, keep: int | None = None) -> list:
        """-> [(program, port, seq, data)] this frame closes, in order; keep: PDUs in front of the fixed-data cut (None: all)"""
        out = []
        nb = index["nbytes"]
        n = min(index["n_pdu"], 16, len(index["pdus"]))
        if keep is not None:
            n = min(n, keep)
        for d in index["pdus"][:n]:
            if d["skipped"]:
                continue
            off, ln = d["psd_off"], d["psd_len"]
            if ln < 0 or off >= nb:
                ln = 0
            ln = min(ln, nb - min(off, nb))
            self.stats["pdus"] += 1
            self.stats["span_bytes"] += ln
            out += self.push_bytes(d["prog_num"], bytes(bytearray(pdu_bytes[off:off + ln])))
        return out


def packet_bytes(pkt) -> bytes:
    """(program, port, seq, data) or (stream, program, port, seq, data) -> the AAS packet as output_aas_push gets it (an `l2aas` record)"""
    port, seq, data = pkt[-3:]
    return bytes([port & 0xFF, port >> 8, seq & 0xFF, seq >> 8]) + bytes(data)
