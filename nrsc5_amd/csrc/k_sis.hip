// Station information service on the device: pids_frame_push + sis_decode (pids.c:935-1050) over the 80-bit PIDS frames the block records
// carry.  The frames never needed the host; what the host gets is one event per state change the reference reports.
//   bit reversal per byte, CRC-12, type bit                                              pids.c:52-86, 1032-1050
//   payload walk: bits[0] + 1 payloads, payload_sizes, `off > 59`, `off > 63 - size`       pids.c:47-50, 935-1019
//   the ten message ids                                                                  pids.c:394-933
//   pids_t                                                                               pids.h:41-96   -> SisState, per consumer stream, in HBM
// One wave64 workgroup per stream of the call; a stream's entries are taken 64 per chunk, in two phases.
//   frame-parallel: one lane per frame.  The packed frame IS the logical bit stream in bytes, most significant bit first (the per-byte reversal
//   of pids.c:1036-1039 and the record's least-significant-first packing cancel), so a field is a shift of two 64-bit words.  Each lane checks the
//   CRC-12 and the type, walks the payloads and leaves at most two ops (message id + the extracted fields, text bytes packed four to a word) in LDS.
//   Everything is integer: latitude and longitude stay the signed 22-bit integers (the host divides by 8192 in float32, which is exact, so equality
//   of the integers is equality of the reference's floats); NaN is the have_lat / have_lon flag.
//   in order: lane 0 applies the ops frame by frame to the stream's state, which the workgroup holds in LDS for the launch (loaded from and stored to
//   HBM by all lanes).  Deliberately serial and plain: at most 16 frames per L1 frame and stream arrive, the stores are single bytes, and the
//   completeness loops are at most 64 steps.
// Events go to a packet arena as in k_psd: SisEvent, then the raw text bytes padded to 4; bump-allocated with the size checked before the first
// byte is written (too small: ArenaHdr::overflow, which the host turns into NRSC5HIP_EOVERFLOW).  Text is not converted here: the event carries
// the encoding and the bytes (strlen-cut where the reference uses strlen), the host decodes.
// Bounds: every index into the text buffers is bounded by the width of the field it is made from (long name 7 * 7 + 6 = 55 < 60, message
// 31 * 6 + 3 = 189 < 192, universal short name frame < 2, slogan 15 * 6 + 4 = 94 < 96, alert 63 * 6 + 2 = 380 < 384); entries outside the list and
// targets outside the consumer are rejected by the host and checked again here.
// Deviations from the reference: its completeness loops run past message_have_frame[32] for message_len >= 191, past slogan_have_frame[16] for
// slogan_len >= 96 and past alert_have_frame[64] for alert_len >= 382 (lengths no set of frames can carry: 32 frames hold 190, 16 hold 95, 64 hold
// 381 bytes).  Here such an item is never complete, and each attempt is counted (SIS_C_NC_*).  The lengths are checked when an item completes only: a
// frame 0 with the same seq rewrites msg_len / slogan_len / alert_len / alert_cnt_len of a displayed item, as in the reference, whose report() then
// reads past its arrays; no event uses them in that state, and the snapshot (nrsc5hip_sis_get) clamps them to 190 / 95 / 381 bytes.
#include <hip/hip_runtime.h>
#include "nrsc5hip.h"
#include "kernels.h"

namespace nrsc5 {

struct SisOp { int f[8]; };                                     // f[0]: message id, f[1..7]: its fields
struct SisParsed { int status, nops, stop; SisOp op[2]; };      // status: 0 bad CRC, 1 LLDS, 2 SIS, -1 no frame; stop: 1 unknown id, 2 no room
struct SisSmem { SisState st; SisParsed fr[64]; unsigned cnt[SIS_STATS]; };

struct SisBits {
    unsigned long long hi, lo;                                  // logical bits 0..63, 64..79 (in the top 16 bits of lo)
    __host__ __device__ unsigned get(int off, int len) const    // decode_int: bits [off, off + len), first bit most significant; 1 <= len <= 32
    {
        const unsigned long long v = off < 64 ? (hi << off) | (off ? lo >> (64 - off) : 0ull) : lo << (off - 64);
        return (unsigned)(v >> (64 - len));
    }
};

__host__ __device__ static void sis_init(SisState &s)           // pids_init, pids.c:1052-1102
{
    uint32_t *w = (uint32_t *)&s;
    for (unsigned k = 0; k < sizeof(SisState) / 4; k++) w[k] = 0u;
    s.fcc = -1; s.long_seq = -1; s.msg_seq = -1;
    for (int i = 0; i < 8; i++) for (int k = 0; k < 3; k++) s.asd[i][k] = -1;
    for (int i = 0; i < 16; i++) for (int k = 0; k < 3; k++) s.dsd[i][k] = -1;
    for (int i = 0; i < 13; i++) s.params[i] = -1;
    s.usn_append = -1; s.usn_len = -1; s.slogan_len = -1; s.alert_seq = -1;
}
void sis_state_init(SisState &s) { sis_init(s); }

__device__ static void sis_text(SisOp &o, const SisBits &b, int off, int n, int width)     // n fields of `width` bits -> bytes of f[4..]
{
    for (int k = 0; k < n; k++) o.f[4 + (k >> 2)] |= (int)(b.get(off + k * width, width) << (8 * (k & 3)));
}

__device__ static void sis_parse(const SisFrame &f, SisParsed &p)
{
    const char *chars = "ABCDEFGHIJKLMNOPQRSTUVWXYZ ?-*$ ";
    const int sizes[16] = {32, 22, 58, 32, 27, 58, 27, 22, 58, 58, 27, -1, -1, -1, -1, -1};
    p.status = 0; p.nops = 0; p.stop = 0;
    if (f.flags & 2u) { p.status = -1; return; }
    SisBits b;
    b.hi = __builtin_bswap64((unsigned long long)f.w[0] | ((unsigned long long)f.w[1] << 32));
    b.lo = __builtin_bswap64((unsigned long long)(f.w[2] & 0xffffu));
    unsigned reg = 0;                                            // crc12, pids.c:52-73
    for (int i = 67; i >= 0; i--) {
        const unsigned low = reg & 1u;
        reg = (reg >> 1) ^ (b.get(i, 1) << 15);
        if (low) reg ^= 0xD010u;
    }
    for (int i = 0; i < 16; i++) { const unsigned low = reg & 1u; reg >>= 1; if (low) reg ^= 0xD010u; }
    if (((reg ^ 0x955u) & 0xfffu) != b.get(68, 12)) return;
    if (b.get(0, 1)) { p.status = 1; return; }
    p.status = 2;
    // sis_decode works on pids + 1: its offset `off` is logical bit off + 1
    const int payloads = (int)b.get(1, 1) + 1;
    int off = 1;
    for (int i = 0; i < payloads; i++) {
        if (off > 59) break;
        const int id = (int)b.get(off + 1, 4);
        off += 4;
        const int size = sizes[id];
        if (size < 0) { p.stop = 1; break; }
        if (off > 63 - size) { p.stop = 2; break; }
        SisOp &o = p.op[p.nops++];
        for (int k = 0; k < 8; k++) o.f[k] = 0;
        o.f[0] = id;
        const int q = off + 1;
        switch (id) {
        case 0:
            o.f[1] = chars[b.get(q, 5)] | (chars[b.get(q + 5, 5)] << 8);
            o.f[2] = (int)b.get(q + 13, 19);
            break;
        case 1:
            for (int k = 0; k < 4; k++) o.f[4] |= chars[b.get(q + 5 * k, 5)] << (8 * k);
            o.f[1] = b.get(q + 20, 1) == 0u && b.get(q + 21, 1) == 1u;
            break;
        case 2:
            o.f[1] = (int)b.get(q, 3); o.f[2] = (int)b.get(q + 3, 3); o.f[3] = (int)b.get(q + 55, 3);
            sis_text(o, b, q + 6, 7, 7);
            break;
        case 4: {
            int v = (int)b.get(q + 1, 22);
            if (v & (1 << 21)) v -= 1 << 22;
            o.f[1] = (int)b.get(q, 1); o.f[2] = v; o.f[3] = (int)b.get(q + 23, 4);
            break; }
        case 5:
            o.f[1] = (int)b.get(q, 5); o.f[2] = (int)b.get(q + 5, 2);
            if (o.f[1] == 0) {
                o.f[3] = (int)(b.get(q + 7, 1) | (b.get(q + 8, 3) << 8) | (b.get(q + 11, 8) << 16) | (b.get(q + 19, 7) << 24));
                sis_text(o, b, q + 26, 4, 8);
            } else sis_text(o, b, q + 10, 6, 8);
            break;
        case 6: case 10:
            o.f[1] = (int)b.get(q, 2);
            o.f[2] = (int)b.get(q + 2, 1);
            if (o.f[1] == 0) { o.f[3] = (int)b.get(q + 3, 6); o.f[4] = (int)b.get(q + 9, 8); o.f[5] = (int)b.get(q + 22, 5); }
            else if (o.f[1] == 1) { o.f[3] = (int)b.get(q + 3, 9); o.f[4] = (int)b.get(q + 15, 12); }
            break;
        case 7:
            o.f[1] = (int)b.get(q, 6); o.f[2] = (int)b.get(q + 6, 16);
            break;
        case 8:
            o.f[1] = (int)b.get(q, 4); o.f[2] = (int)b.get(q + 4, 1);
            if (o.f[1] != 0) sis_text(o, b, q + 10, 6, 8);
            else if (o.f[2] == 0) { o.f[3] = (int)(b.get(q + 5, 3) | (b.get(q + 8, 1) << 8) | ((b.get(q + 9, 1) + 1u) << 16)); sis_text(o, b, q + 10, 6, 8); }
            else { o.f[3] = (int)(b.get(q + 5, 3) | (b.get(q + 11, 7) << 8)); sis_text(o, b, q + 18, 5, 8); }
            break;
        case 9:
            o.f[1] = (int)b.get(q, 6); o.f[2] = (int)b.get(q + 6, 2);
            if (o.f[1] == 0) {
                o.f[3] = (int)(b.get(q + 10, 3) | (b.get(q + 13, 9) << 8) | (b.get(q + 22, 7) << 20));
                o.f[6] = 1 + 2 * (int)b.get(q + 29, 5);
                sis_text(o, b, q + 34, 3, 8);
            } else sis_text(o, b, q + 10, 6, 8);
            break;
        default: break;                                         // 3: reserved
        }
        off += size;
    }
}

// ---- the in-order phase: one lane -----------------------------------------------------------------------------------------------------------
struct SisCtx { const SisArgs *a; SisSmem *sm; unsigned pos, entry; };

__device__ static void sis_emit(SisCtx &c, int kind, int enc, const int *v, int nv, const uint8_t *data, int len)
{
    const SisArgs &a = *c.a;
    const unsigned rec = (unsigned)sizeof(SisEvent) + (((unsigned)len + 3u) & ~3u);
    const unsigned at = arena_reserve(a.hdr, a.arena_cap, rec);
    if (at == ARENA_FULL) return;
    SisEvent e;
    e.pos = c.pos; e.entry = c.entry; e.kind = (uint16_t)kind; e.len = (uint16_t)len; e.enc = enc;
    for (int k = 0; k < 8; k++) e.v[k] = k < nv ? v[k] : 0;
    *(SisEvent *)(a.arena + at) = e;
    uint8_t *d = a.arena + at + (unsigned)sizeof(SisEvent);
    for (unsigned k = 0; k < (((unsigned)len + 3u) & ~3u); k++) d[k] = k < (unsigned)len ? data[k] : (uint8_t)0;
    atomicAdd(&a.hdr->count, 1u);
    c.sm->cnt[SIS_C_EVENTS]++;
}

__device__ static int sis_strlen(const uint8_t *p, int cap) { int n = 0; while (n < cap && p[n]) n++; return n; }
__device__ static void sis_bytes(uint8_t *dst, const SisOp &o, int n) { for (int k = 0; k < n; k++) dst[k] = (uint8_t)(o.f[4 + (k >> 2)] >> (8 * (k & 3))); }

__device__ static int sis_crc7(const uint8_t *alert, int len)   // pids.c:88-117
{
    unsigned reg = 0x42u;
    for (int i = len - 1; i >= 0; i--)
        for (int k = 6; k >= 0; k--) {
            unsigned bit = (alert[i] >> k) & 1u;
            if (k == 0 && i > 0) bit ^= alert[i - 1] >> 7;
            reg = ((reg << 1) ^ bit) & 0xffu;
            if (reg & 0x80u) reg ^= 0x89u;
        }
    for (int k = 6; k >= 0; k--) { reg = (reg << 1) & 0xffu; if (reg & 0x80u) reg ^= 0x89u; }
    return (int)reg;
}

__device__ static int sis_cnt_crc(const uint8_t *cd, int len)   // control_data_crc, pids.c:119-153
{
    unsigned reg = 0x7E1Bu;
    for (int i = len - 1; i >= 1; i--)
        for (int k = 0; k < 8; k++) {
            unsigned bit = (cd[i] >> k) & 1u;
            if (i == 1 || (i == 2 && k < 4)) bit = 0u;
            const unsigned low = reg & 1u;
            reg = (reg >> 1) ^ (bit << 15);
            if (low) reg ^= 0xD010u;
        }
    for (int k = 0; k < 16; k++) { const unsigned low = reg & 1u; reg >>= 1; if (low) reg ^= 0xD010u; }
    return (int)(reg & 0x0fffu);
}

__device__ static void sis_params(SisCtx &c, int index)         // the switch of sis_decode_parameter, pids.c:667-752
{
    const int *p = c.sm->st.params;
    if (index <= 2) {
        if (p[0] >= 0 && p[1] >= 0 && p[2] >= 0) {
            const int v[3] = {p[0] >> 8, p[0] & 0xff, (int)(((unsigned)p[2] << 16) | (unsigned)p[1])};
            sis_emit(c, NRSC5HIP_SIS_LEAP_SECOND, 0, v, 3, nullptr, 0);
        }
    } else if (index == 3) {
        int tzo = (p[3] >> 5) & 0x7ff;
        if (tzo >= 1024) tzo -= 2048;
        const int v[4] = {tzo, p[3] & 1, (p[3] >> 1) & 1, (p[3] >> 2) & 7};
        sis_emit(c, NRSC5HIP_SIS_LOCAL_TIME, 0, v, 4, nullptr, 0);
    } else if (index <= 7) {
        if (p[4] >= 0 && p[5] >= 0 && p[6] >= 0 && p[7] >= 0) sis_emit(c, NRSC5HIP_SIS_EXCITER, 0, p + 4, 4, nullptr, 0);
    } else if (index <= 11) {
        if (p[8] >= 0 && p[9] >= 0 && p[10] >= 0 && p[11] >= 0) sis_emit(c, NRSC5HIP_SIS_IMPORTER, 0, p + 8, 4, nullptr, 0);
    }
}

__device__ static void sis_apply(SisCtx &c, const SisOp &o)
{
    SisState &s = c.sm->st;
    unsigned *cnt = c.sm->cnt;
    switch (o.f[0]) {
    case 0:                                                     // pids.c:394-417
        if (o.f[1] != s.cc || o.f[2] != s.fcc) {
            s.cc = o.f[1]; s.fcc = o.f[2];
            const uint8_t cc[2] = {(uint8_t)(s.cc & 0xff), (uint8_t)(s.cc >> 8)};
            sis_emit(c, NRSC5HIP_SIS_STATION_ID, 0, &s.fcc, 1, cc, 2);
        }
        break;
    case 1: {                                                   // pids.c:419-440
        uint8_t name[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        sis_bytes(name, o, 4);
        if (o.f[1]) { name[4] = '-'; name[5] = 'F'; name[6] = 'M'; }
        bool same = true;
        for (int k = 0; k < 8; k++) same = same && name[k] == s.short_name[k];
        if (!same) {
            for (int k = 0; k < 8; k++) s.short_name[k] = name[k];
            sis_emit(c, NRSC5HIP_SIS_STATION_NAME, 0, nullptr, 0, s.short_name, o.f[1] ? 7 : 4);
        }
        break; }
    case 2: {                                                   // pids.c:442-485
        const int last = o.f[1], cur = o.f[2], seq = o.f[3];
        if (cur == 0 && seq != s.long_seq) {
            for (int k = 0; k < 60; k++) s.long_name[k] = 0;
            for (int k = 0; k < 8; k++) s.long_have[k] = 0;
            s.long_seq = seq; s.long_displayed = 0;
        }
        sis_bytes(s.long_name + cur * 7, o, 7);
        s.long_have[cur] = 1;
        if (s.long_seq >= 0 && !s.long_displayed) {
            int complete = 1;
            for (int k = 0; k < last + 1; k++) complete &= s.long_have[k];
            if (complete) {
                s.long_displayed = 1;
                if (!s.slogan_displayed) sis_emit(c, NRSC5HIP_SIS_STATION_SLOGAN, 0, nullptr, 0, s.long_name, sis_strlen(s.long_name, 56));
            }
        }
        break; }
    case 4:                                                     // pids.c:487-523
        if (o.f[1]) {
            const int high = o.f[3] << 8;
            if (!s.have_lat || o.f[2] != s.lat || high != (s.altitude & 0xf00)) {
                s.lat = o.f[2]; s.have_lat = 1; s.altitude = (s.altitude & 0x0f0) | high;
                if (s.have_lon) { const int v[3] = {s.lat, s.lon, s.altitude}; sis_emit(c, NRSC5HIP_SIS_STATION_LOCATION, 0, v, 3, nullptr, 0); }
            }
        } else {
            const int low = o.f[3] << 4;
            if (!s.have_lon || o.f[2] != s.lon || low != (s.altitude & 0x0f0)) {
                s.lon = o.f[2]; s.have_lon = 1; s.altitude = (s.altitude & 0xf00) | low;
                if (s.have_lat) { const int v[3] = {s.lat, s.lon, s.altitude}; sis_emit(c, NRSC5HIP_SIS_STATION_LOCATION, 0, v, 3, nullptr, 0); }
            }
        }
        break;
    case 5: {                                                   // pids.c:525-586
        const int cur = o.f[1], seq = o.f[2];
        if (cur == 0) {
            if (seq != s.msg_seq) {
                for (int k = 0; k < 192; k++) s.message[k] = 0;
                for (int k = 0; k < 32; k++) s.msg_have[k] = 0;
                s.msg_seq = seq; s.msg_displayed = 0;
            }
            s.msg_priority = o.f[3] & 1; s.msg_enc = (o.f[3] >> 8) & 7; s.msg_len = (o.f[3] >> 16) & 0xff; s.msg_checksum = (o.f[3] >> 24) & 0x7f;
            sis_bytes(s.message, o, 4);
        } else sis_bytes(s.message + cur * 6 - 2, o, 6);
        s.msg_have[cur] = 1;
        if (s.msg_seq >= 0 && !s.msg_displayed) {
            const int need = (s.msg_len + 7) / 6;
            if (need > 32) { cnt[SIS_C_NC_MESSAGE]++; break; }
            int complete = 1;
            for (int k = 0; k < need; k++) complete &= s.msg_have[k];
            if (complete) {
                unsigned sum = 0;
                for (int k = 0; k < s.msg_len; k++) sum += s.message[k];
                sum = (((sum >> 8) & 0x7fu) + (sum & 0xffu)) & 0x7fu;
                if ((int)sum == s.msg_checksum) {
                    s.msg_displayed = 1;
                    sis_emit(c, NRSC5HIP_SIS_STATION_MESSAGE, s.msg_enc, &s.msg_priority, 1, s.message, s.msg_len);
                } else cnt[SIS_C_BAD_CHECKSUM]++;
            }
        }
        break; }
    case 6: case 10:                                            // pids.c:588-649
        if (o.f[1] == 0) {
            const int prog = o.f[3];
            if (prog >= 8) break;
            int *d = s.asd[prog];
            if (d[0] != o.f[2] || d[1] != o.f[4] || d[2] != o.f[5]) {
                d[0] = o.f[2]; d[1] = o.f[4]; d[2] = o.f[5];
                const int v[4] = {prog, d[0], d[1], d[2]};
                sis_emit(c, NRSC5HIP_SIS_AUDIO_SERVICE, 0, v, 4, nullptr, 0);
            }
        } else if (o.f[1] == 1) {
            for (int k = 0; k < 16; k++) {
                int *d = s.dsd[k];
                if (d[0] == o.f[2] && d[1] == o.f[3] && d[2] == o.f[4]) break;
                if (d[1] == -1) {
                    d[0] = o.f[2]; d[1] = o.f[3]; d[2] = o.f[4];
                    sis_emit(c, NRSC5HIP_SIS_DATA_SERVICE, 0, d, 3, nullptr, 0);
                    break;
                }
            }
        }
        break;
    case 7:                                                     // pids.c:651-754
        if (o.f[1] < 13 && s.params[o.f[1]] != o.f[2]) { s.params[o.f[1]] = o.f[2]; sis_params(c, o.f[1]); }
        break;
    case 8: {                                                   // pids.c:756-851
        const int cur = o.f[1];
        if (o.f[2] == 0) {
            if (cur >= 2) break;
            if (cur == 0) { s.usn_enc = o.f[3] & 7; s.usn_append = (o.f[3] >> 8) & 1; s.usn_len = (o.f[3] >> 16) & 3; }
            sis_bytes(s.usn + cur * 6, o, 6);
            s.usn_have[cur] = 1;
            if (s.usn_len >= 0 && !s.usn_displayed) {
                int complete = 1;
                for (int k = 0; k < s.usn_len; k++) complete &= s.usn_have[k];
                if (complete) {
                    int n = sis_strlen(s.usn, 12);
                    for (int k = 0; k < n; k++) s.usn_final[k] = s.usn[k];
                    if (s.usn_append) { s.usn_final[n] = '-'; s.usn_final[n + 1] = 'F'; s.usn_final[n + 2] = 'M'; n += 3; }
                    s.usn_final[n] = 0;
                    s.usn_displayed = 1;
                    sis_emit(c, NRSC5HIP_SIS_STATION_NAME, s.usn_enc, nullptr, 0, s.usn_final, n);
                }
            }
        } else {
            if (cur == 0) { s.slogan_enc = o.f[3] & 7; s.slogan_len = (o.f[3] >> 8) & 0x7f; sis_bytes(s.slogan, o, 5); }
            else sis_bytes(s.slogan + cur * 6 - 1, o, 6);
            s.slogan_have[cur] = 1;
            if (s.slogan_len >= 0 && !s.slogan_displayed) {
                const int need = (s.slogan_len + 6) / 6;
                if (need > 16) { cnt[SIS_C_NC_SLOGAN]++; break; }
                int complete = 1;
                for (int k = 0; k < need; k++) complete &= s.slogan_have[k];
                if (complete) {
                    s.slogan_displayed = 1;
                    if (!s.long_displayed) sis_emit(c, NRSC5HIP_SIS_STATION_SLOGAN, s.slogan_enc, nullptr, 0, s.slogan, s.slogan_len);
                }
            }
        }
        break; }
    case 9: {                                                   // pids.c:853-933
        const int cur = o.f[1], seq = o.f[2];
        s.alert_timeout = 0;
        if (cur == 0) {
            if (seq != s.alert_seq) {
                for (int k = 0; k < 384; k++) s.alert[k] = 0;
                for (int k = 0; k < 64; k++) s.alert_have[k] = 0;
                s.alert_seq = seq; s.alert_displayed = 0;
            }
            s.alert_enc = o.f[3] & 7; s.alert_len = (o.f[3] >> 8) & 0x1ff; s.alert_crc = (o.f[3] >> 20) & 0x7f; s.alert_cnt_len = o.f[6];
            sis_bytes(s.alert, o, 3);
        } else sis_bytes(s.alert + cur * 6 - 3, o, 6);
        s.alert_have[cur] = 1;
        if (s.alert_len >= 0 && !s.alert_displayed) {
            const int need = (s.alert_len + 8) / 6;
            if (need > 64) { cnt[SIS_C_NC_ALERT]++; break; }
            int complete = 1;
            for (int k = 0; k < need; k++) complete &= s.alert_have[k];
            if (complete) {
                if (s.alert_crc != sis_crc7(s.alert, s.alert_len)) { cnt[SIS_C_BAD_CRC7]++; break; }
                if (s.alert_cnt_len < 7 || s.alert_len < s.alert_cnt_len) { cnt[SIS_C_BAD_CNT_LEN]++; break; }
                const int actual = ((s.alert[2] & 0x0f) << 8) | s.alert[1];
                if (actual == sis_cnt_crc(s.alert, s.alert_cnt_len)) {
                    s.alert_displayed = 1;
                    sis_emit(c, NRSC5HIP_SIS_ALERT, s.alert_enc, &s.alert_cnt_len, 1, s.alert, s.alert_len);
                } else cnt[SIS_C_BAD_CNT_CRC]++;
            }
        }
        break; }
    default: break;
    }
}

__device__ static void sis_frame(SisCtx &c, const SisFrame &f, const SisParsed &p)
{
    SisState &s = c.sm->st;
    unsigned *cnt = c.sm->cnt;
    if (f.flags & 1u) sis_init(s);                              // decode_reset, sync.c:407
    if (p.status < 0) return;
    cnt[SIS_C_FRAMES]++;
    if (p.status == 0) return;
    cnt[SIS_C_CRC]++;
    if (p.status == 1) { cnt[SIS_C_LLDS]++; return; }
    cnt[SIS_C_SIS]++;
    if (s.alert_displayed) s.alert_timeout++;
    for (int k = 0; k < p.nops; k++) { cnt[SIS_C_ID0 + (p.op[k].f[0] & 15)]++; sis_apply(c, p.op[k]); }
    if (p.stop == 1) cnt[SIS_C_UNKNOWN]++;
    if (p.stop == 2) cnt[SIS_C_NOROOM]++;
    if (s.alert_displayed && s.alert_timeout >= 16) {           // reset_alert, pids.c:385-392, 1021-1026
        for (int k = 0; k < 384; k++) s.alert[k] = 0;
        for (int k = 0; k < 64; k++) s.alert_have[k] = 0;
        s.alert_seq = -1; s.alert_displayed = 0; s.alert_timeout = 0;
        const int v[1] = {-1};
        sis_emit(c, NRSC5HIP_SIS_ALERT, 0, v, 1, nullptr, 0);
    }
}

__global__ __launch_bounds__(64) void k_sis(SisArgs a)
{
    __shared__ SisSmem sm;
    const int lane = (int)threadIdx.x;
    const ArenaStream s = a.streams[blockIdx.x];
    if (s.target < 0 || s.target >= a.nstreams) return;          // (wave-uniform: the whole workgroup leaves)
    uint32_t *gs = (uint32_t *)(a.state + s.target), *ls = (uint32_t *)&sm.st;
    for (unsigned k = (unsigned)lane; k < sizeof(SisState) / 4; k += 64u) ls[k] = gs[k];
    if (lane < SIS_STATS) sm.cnt[lane] = 0u;
    __syncthreads();
    for (int base = 0; base < s.count; base += 64) {
        const int n = s.count - base < 64 ? s.count - base : 64;
        const int e = s.first + base + lane;
        if (lane < n) {
            if (e >= 0 && e < a.nentries) sis_parse(a.frames[e], sm.fr[lane]);
            else { sm.fr[lane].status = -1; sm.fr[lane].nops = 0; sm.fr[lane].stop = 0; }
        }
        __syncthreads();
        if (lane == 0) {
            SisCtx c{&a, &sm, (unsigned)s.pos, 0u};
            for (int k = 0; k < n; k++) {
                const int ek = s.first + base + k;
                if (ek < 0 || ek >= a.nentries) break;
                c.entry = (unsigned)(base + k);
                sis_frame(c, a.frames[ek], sm.fr[k]);
            }
        }
        __syncthreads();
    }
    for (unsigned k = (unsigned)lane; k < sizeof(SisState) / 4; k += 64u) gs[k] = ls[k];
    if (lane < SIS_STATS) a.stats[(size_t)s.target * SIS_STATS + lane] += sm.cnt[lane];
}

void launch_sis(const SisArgs &a, int nstreams, hipStream_t st)
{
    if (nstreams < 1) return;
    hipLaunchKernelGGL(k_sis, dim3(nstreams), dim3(64), 0, st, a);
}

}  // namespace nrsc5
