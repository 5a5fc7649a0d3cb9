// PSD transport on the device: parse_hdlc + aas_push (frame.c:328-391) over the PSD spans the L2 index marks, as a post-pass over the
// index structs and RS-corrected PDU bytes k_l2_index left in HBM.  The frames never reach the host: finished AAS packets do.
//   parse_hdlc over [psd_off, psd_off + psd_len) of every walked PDU, per program         frame.c:369-391, 611
//   unescape_hdlc (0x7D takes the next byte OR 0x20), fcs16, protocol byte 0x21          frame.c:328-366
//   frame_t.psd_buf / psd_idx                                                            frame.h:5,44-45   -> PsdArgs::bufs / idx, per (stream, program)
// One wave64 workgroup per stream of the call: it walks that stream's jobs in order, so the state of a stream has one writer and the
// order of its packets is the order of the bytes.  Workgroups never wait for each other.
//
// A span is taken 64 bytes per step.  __ballot gives the mask of flag bytes (0x7E); the bytes between two flags are one contiguous piece
// of the open frame, stored raw at idx + (lane - first lane of the piece), as the reference stores them raw; every lane derives the same
// idx from the same masks, so all control flow is wave-uniform.  At a flag the frame buf[0, idx) is closed: read back 64 bytes per step,
// a second ballot marks the 0x7D bytes, the parity of each lane's position inside its run of 0x7D (carried over the step boundary) says
// which of them are escape markers, and the popcount of the kept lanes below gives each byte's place in the unescaped copy in LDS.
// FCS-16 runs over that copy from a table, serially (frames close a few times per second and program), then the packet goes to the arena.
//
// Bounds: every span is clamped to the frame's nbytes and to the stride of the byte buffer; a job's frame index is checked against the
// frame count; idx stays in [-1, 8212] by construction (a piece is cut at the room left); the arena is bump-allocated with the size
// checked before the first byte is written (too small: ArenaHdr::overflow, which the host turns into an error).
// Deviations from the reference: a frame whose last raw byte is an unpaired 0x7D is dropped (the reference ORs one stale byte of its
// buffer into the frame; such a frame fails its FCS in practice); a packet shorter than port + seq (4 bytes), for which the reference's
// output_aas_push reads past the packet, is dropped as "wrong protocol".
#include <hip/hip_runtime.h>
#include "nrsc5hip.h"
#include "kernels.h"

namespace nrsc5 {

struct PsdSmem {
    uint16_t fcs_tab[256];
    uint8_t out[PSD_MAX_AAS + 4];     // the unescaped copy of the frame being closed
    int idx[PSD_PROGRAMS];
};

struct PsdCount { unsigned long long v[PSD_STATS]; };
enum { PSD_C_PDUS = 0, PSD_C_BYTES, PSD_C_CLOSED, PSD_C_EMPTY, PSD_C_FCS, PSD_C_PROTOCOL, PSD_C_TRUNCATED, PSD_C_OVERFLOW, PSD_C_DELIVERED };

// aas_push on the raw frame buf[0, n), n >= 0; wave-uniform
__device__ inline void psd_close(PsdSmem &sm, const PsdArgs &a, const ArenaStream &s, const uint8_t *buf, int n, unsigned program, PsdCount &c)
{
    const int lane = (int)threadIdx.x;
    const unsigned long long low = (1ull << lane) - 1ull;
    const volatile uint8_t *raw = buf;                          // bytes this wave stored a moment ago: read past the vector L1
    c.v[PSD_C_CLOSED]++;
    __syncthreads();                                            // ... and behind those stores; also: the previous close is done with sm.out
    int outn = 0;
    bool carry = false;                                         // the last byte of the previous step was an escape marker
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool valid = i < n;
        const unsigned b = valid ? raw[i] : 0u;
        const unsigned long long vm = __ballot(valid), em = __ballot(valid && b == 0x7Du);
        const unsigned long long others = ~em & low;            // lanes below this one that do not hold 0x7D
        const int start = others ? 64 - __builtin_clzll(others) : 0;                 // first lane of the run of 0x7D this lane is in
        const int ri = lane - start + ((start == 0 && carry) ? 1 : 0);               // position in the run: even = marker, odd = escaped 0x7D
        const bool marker = valid && b == 0x7Du && !(ri & 1);
        const unsigned long long mk = __ballot(marker);
        const bool escaped = lane ? ((mk >> (lane - 1)) & 1ull) != 0 : carry;
        if (valid && !marker) sm.out[outn + __popcll(~mk & vm & low)] = (uint8_t)(escaped ? (b | 0x20u) : b);
        outn += __popcll(~mk & vm);
        carry = ((mk >> (__popcll(vm) - 1)) & 1ull) != 0;
    }
    __syncthreads();
    if (carry) { c.v[PSD_C_TRUNCATED]++; return; }
    if (outn == 0) { c.v[PSD_C_EMPTY]++; return; }
    unsigned crc = 0xffffu;                                     // fcs16, frame.c:138-144; every lane the same walk (LDS broadcast reads)
    for (int i = 0; i < outn; i++) crc = (crc >> 8) ^ sm.fcs_tab[(crc ^ sm.out[i]) & 0xffu];
    if (crc != 0xf0b8u) { c.v[PSD_C_FCS]++; return; }
    if (sm.out[0] != 0x21u || outn < 7) { c.v[PSD_C_PROTOCOL]++; return; }
    const unsigned len = (unsigned)outn - 7u;                   // protocol byte, port, seq in front; FCS behind
    const unsigned rec = (unsigned)sizeof(PsdPacket) + ((len + 3u) & ~3u);
    unsigned at = 0;
    if (lane == 0) at = arena_reserve(a.hdr, a.arena_cap, rec);
    at = __shfl(at, 0);
    if (at == ARENA_FULL) return;
    if (lane == 0) {
        PsdPacket p;
        p.pos = (uint32_t)s.pos; p.port = (uint16_t)(sm.out[1] | (sm.out[2] << 8)); p.seq = (uint16_t)(sm.out[3] | (sm.out[4] << 8));
        p.len = (uint16_t)len; p.program = (uint8_t)program; p.pad = 0;
        *(PsdPacket *)(a.arena + at) = p;
        atomicAdd(&a.hdr->count, 1u);
    }
    for (unsigned i = (unsigned)lane; i < len; i += 64u) a.arena[at + (unsigned)sizeof(PsdPacket) + i] = sm.out[5u + i];
    c.v[PSD_C_DELIVERED]++;
}

__global__ __launch_bounds__(64) void k_psd(PsdArgs a)
{
    __shared__ PsdSmem sm;
    const int lane = (int)threadIdx.x;
    const ArenaStream s = a.streams[blockIdx.x];
    for (int k = lane; k < 256; k += 64) {                      // the table of frame.c:92-125: reflected 0x8408
        unsigned v = (unsigned)k;
        for (int j = 0; j < 8; j++) v = (v & 1u) ? (v >> 1) ^ 0x8408u : v >> 1;
        sm.fcs_tab[k] = (uint16_t)v;
    }
    int *gidx = a.idx + (size_t)s.target * PSD_PROGRAMS;
    uint8_t *gbuf = a.bufs + (size_t)s.target * PSD_PROGRAMS * PSD_MAX_AAS;
    if (lane < PSD_PROGRAMS) { const int v = gidx[lane]; sm.idx[lane] = (v < -1 || v > PSD_MAX_AAS) ? -1 : v; }
    __syncthreads();
    PsdCount c;
    for (int k = 0; k < PSD_STATS; k++) c.v[k] = 0;

    for (int j = 0; j < s.count; j++) {
        const int jn = s.first + j;
        if (jn < 0 || jn >= a.njobs) break;
        const PsdJob job = a.jobs[jn];
        if (job.reset) {                                        // frame_reset, frame.c:730-733
            __syncthreads();
            if (lane < PSD_PROGRAMS) sm.idx[lane] = -1;
            __syncthreads();
        }
        if (job.frame < 0 || job.frame >= a.nframes) continue;
        const nrsc5hip_l2_frame &fr = a.frames[job.frame];
        const uint8_t *src = a.bytes + (long long)job.frame * a.stride;
        unsigned nb = fr.nbytes;
        if ((long long)nb > a.stride) nb = (unsigned)a.stride;
        unsigned npdu = fr.n_pdu;
        if (npdu > (unsigned)NRSC5HIP_L2_MAX_PDUS) npdu = NRSC5HIP_L2_MAX_PDUS;
        if (job.keep >= 0 && npdu > (unsigned)job.keep) npdu = (unsigned)job.keep;
        for (unsigned q = 0; q < npdu; q++) {
            const nrsc5hip_l2_pdu &pd = fr.pdu[q];
            if (pd.skipped || pd.prog_num >= PSD_PROGRAMS) continue;
            const unsigned program = pd.prog_num, off = pd.psd_off;
            int len = pd.psd_len;
            if (len < 0 || off >= nb) len = 0;
            if ((unsigned)len > nb - (off < nb ? off : nb)) len = (int)(nb - off);
            c.v[PSD_C_PDUS]++; c.v[PSD_C_BYTES] += (unsigned)len;
            uint8_t *buf = gbuf + (size_t)program * PSD_MAX_AAS;
            int idx = sm.idx[program];
            for (int base = 0; base < len; base += 64) {
                const int n = len - base < 64 ? len - base : 64;
                const bool valid = lane < n;
                const unsigned b = valid ? src[off + (unsigned)(base + lane)] : 0u;
                const unsigned long long fm = __ballot(valid && b == 0x7Eu);
                int pos = 0;                                    // first lane of the piece in front of the next flag
                for (;;) {
                    const unsigned long long rem = pos < 64 ? (fm >> pos) << pos : 0ull;
                    const int end = rem ? __builtin_ctzll(rem) : n;
                    const int cnt = end - pos;
                    if (cnt > 0 && idx >= 0) {
                        const int room = PSD_MAX_AAS - idx, take = cnt < room ? cnt : room;
                        if (lane >= pos && lane < pos + take) buf[idx + lane - pos] = (uint8_t)b;
                        if (cnt > room) { idx = -1; c.v[PSD_C_OVERFLOW]++; }      // the byte that finds idx == 8212 closes the frame unseen, frame.c:382-387
                        else idx += cnt;
                    }
                    if (!rem) break;
                    if (idx >= 0) psd_close(sm, a, s, buf, idx, program, c);
                    idx = 0;
                    pos = end + 1;
                }
            }
            __syncthreads();                                    // every lane has read sm.idx[program]
            if (lane == 0) sm.idx[program] = idx;
            __syncthreads();
        }
    }
    __syncthreads();
    if (lane < PSD_PROGRAMS) gidx[lane] = sm.idx[lane];
    if (lane == 0) {
        unsigned long long *st = a.stats + (size_t)s.target * PSD_STATS;
        for (int k = 0; k < PSD_STATS; k++) st[k] += c.v[k];
    }
}

void launch_psd(const PsdArgs &a, int nstreams, hipStream_t st)
{
    if (nstreams < 1) return;
    hipLaunchKernelGGL(k_psd, dim3(nstreams), dim3(64), 0, st, a);
}

}  // namespace nrsc5
