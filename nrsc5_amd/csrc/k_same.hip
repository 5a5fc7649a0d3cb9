// EAS alerts (SAME headers and end-of-message bursts) in a station's analog audio, from the discriminator output d[m] at Fs1 = 372 093.75 S/s
// (include/nrsc5hip.h, "SAME"; the definition: DESIGN.md (s)).  Every quantity is a function of absolute sample indices, no recurrence in the
// signal path: any chunking gives the same bits, events and counters.
//   k_same_tones   one wave = TT = 64 consecutive segments of one channel (8 per bit, segment r = samples [35721 r / 400, 35721 (r + 1) / 400)).
//                  The d span of the tile (5715 or 5716 floats) is staged in LDS by coalesced loads; lane = segment sums its 89 or 90 samples in
//                  ascending m against the two exact phasors ((200 m) mod 35721 and (150 m) mod 35721 index one table).  Neighbouring lanes
//                  start 89 or 90 floats apart in LDS: an odd stride most of the time, few bank conflicts.
//   k_same_bits    one wave = one complete window of 64 bits: q of its 512 grid points (lane l takes points l, l + 64, ..; each the 8 segment
//                  sums added in order) into LDS, the 8 timing metrics (8 terms per lane in order, then a butterfly), s_w, the seam rule
//                  against s_{w-1} (kept from the last call, or formed again from the c of window w - 1), and up to 65 decisions q > 0.
//   k_same_frames  one wave = one channel.  Per 64 bits a position-parallel phase (lane = bit position: are the 16 bits that end there
//                  0xAB 0xAB) and an in-order phase on lane 0 (search, preamble, message, the three-burst vote; the state lives in HBM and is
//                  held in LDS for the launch).  Events go to the channel's arena, sized by the host from the bits.
//   k_same_keep    the c of the incomplete window move to the front of the other buffer.
#include <hip/hip_runtime.h>
#include "fm_audio.h"
#include "same.h"

namespace nrsc5 {
namespace same {
namespace {

__global__ __launch_bounds__(64) void k_same_tones(TonesArgs a)
{
    __shared__ float ds[TONE_SPAN];
    const int ch = blockIdx.y, lane = threadIdx.x;
    const long long rt0 = a.r0 + (long long)blockIdx.x * TT;
    const long long left = a.r0 + a.r_count - rt0;
    const int cnt = left < TT ? (int)left : TT;
    if (cnt <= 0) return;
    const long long m_lo = grid_floor(rt0);                   // ds[k] = d[m_lo + k]
    const int span = (int)(grid_floor(rt0 + cnt) - m_lo);     // <= TONE_SPAN - 1
    const float *d = a.d + (long long)ch * a.d_stride - a.d_base;
    for (int k = lane; k < span; k += 64) ds[k] = d[m_lo + k];
    __syncthreads();
    if (lane < cnt) {
        const long long r = rt0 + lane;
        const long long m0 = grid_floor(r);
        const int n = (int)(grid_floor(r + 1) - m0), off = (int)(m0 - m_lo);
        int k1 = (int)(((long long)K_MARK * m0) % DEN), k0 = (int)(((long long)K_SPACE * m0) % DEN);
        float re1 = 0.0f, im1 = 0.0f, re0 = 0.0f, im0 = 0.0f;
        for (int i = 0; i < n; i++) {
            const float x = ds[off + i];
            const float2 t1 = a.cs[k1], t0 = a.cs[k0];
            re1 = fmaf(x, t1.x, re1); im1 = fmaf(x, t1.y, im1);
            re0 = fmaf(x, t0.x, re0); im0 = fmaf(x, t0.y, im0);
            k1 += K_MARK; if (k1 >= DEN) k1 -= DEN;
            k0 += K_SPACE; if (k0 >= DEN) k0 -= DEN;
        }
        a.c[(long long)ch * a.c_stride + (r - a.c_base)] = make_float4(re1, -im1, re0, -im0);     // d exp(-j phi)
    }
}

// q of the 512 grid points of the window whose first segment sum is c0[0], into qs; lane l takes points l, l + 64, ..
__device__ __forceinline__ void window_q(const float4 *c0, int lane, float *qs)
{
    for (int i = 0; i < WIN_PTS / 64; i++) {
        const int p = lane + 64 * i;
        float4 s = c0[p];
        for (int k = 1; k < S; k++) {
            const float4 v = c0[p + k];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        qs[p] = (s.x * s.x + s.y * s.y) - (s.z * s.z + s.w * s.w);
    }
}

// the 8 timing metrics of the window in qs, lane 8 g + s: bits g, g + 8, .. in order, then a butterfly over g -> argmax, ties to the lowest s
__device__ __forceinline__ int window_timing(const float *qs, int lane, float *metric)
{
    const int s = lane & 7, g = lane >> 3;
    float e = 0.0f;
    for (int k = 0; k < WIN_BITS / 8; k++) e += fabsf(qs[S * (g + 8 * k) + s]);
    for (int st = 8; st <= 32; st <<= 1) e += __shfl_xor(e, st);
    int best = 0;
    float eb = __shfl(e, 0);
    for (int q = 1; q < S; q++) {
        const float eq = __shfl(e, q);
        if (eq > eb) { eb = eq; best = q; }
    }
    *metric = e;
    return best;
}

__global__ __launch_bounds__(64) void k_same_bits(BitsArgs a)
{
    __shared__ float qs[WIN_PTS];
    const int ch = blockIdx.y, wi = blockIdx.x, lane = threadIdx.x;
    const long long w = a.w0 + wi;
    const float4 *c = a.c + (long long)ch * a.c_stride - a.c_base;     // c[r] by its absolute index
    int sp = -1;
    float e;
    if (w > 0) {
        if (wi > 0) {
            window_q(c + (w - 1) * WIN_PTS, lane, qs);
            __syncthreads();
            sp = window_timing(qs, lane, &e);
            __syncthreads();
        } else sp = a.s_in[ch];
    }
    window_q(c + w * WIN_PTS, lane, qs);
    __syncthreads();
    const int sw = window_timing(qs, lane, &e);
    // the window's sampling points, as offsets into it: an inserted point, or the first one dropped, by the gap to the last point of window w - 1
    int ins = 0, drop = 0;
    if (w > 0) {
        const int gap = S + sw - sp;
        if (gap < 4) drop = 1;
        else if (gap > 12) ins = 1;
    }
    const int nb = WIN_BITS + ins - drop;
    uint8_t *bits = a.bits + ((long long)ch * a.nwin + wi) * BITS_STRIDE;
    for (int b = lane; b < BITS_STRIDE; b += 64) {
        uint8_t bit = 0;
        if (b < nb) {
            const int p = ins ? (b == 0 ? sp : S * (b - 1) + sw) : S * (b + drop) + sw;   // (the inserted point: 8 steps behind 512 w - 8 + s_{w-1})
            bit = qs[p] > 0.0f ? 1 : 0;
        }
        bits[b] = bit;
    }
    if (a.q)
        for (int p = lane; p < WIN_PTS; p += 64) a.q[((long long)ch * a.nwin + wi) * WIN_PTS + p] = qs[p];
    if (lane < S && a.metric) a.metric[((long long)ch * a.nwin + wi) * S + lane] = e;
    if (lane == 0) {
        a.counts[(long long)ch * a.nwin + wi] = nb;
        if (a.s_w) a.s_w[(long long)ch * a.nwin + wi] = sw;
        if (wi == a.nwin - 1) a.s_out[ch] = sw;
        if (a.stats) {
            if (drop) atomicAdd(a.stats + (long long)ch * NSTATS + ST_SEAM_DROPS, 1ull);
            if (ins) atomicAdd(a.stats + (long long)ch * NSTATS + ST_SEAM_INSERTS, 1ull);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- framing and the vote
struct FramesSmem {
    State st;
    unsigned long long stats[NSTATS];
    uint8_t win[64 + 15];
    uint8_t match[64];
    int burst_events;
};

struct Emit {                                                           // lane 0's view of the channel's arena
    uint8_t *arena; unsigned *used, *overflow; unsigned cap; int ch;
};

__device__ void emit(FramesSmem &sm, const Emit &o, int kind, long long first, long long last, const int *v, int nv, const unsigned char *data, unsigned len)
{
    const unsigned rec = (unsigned)sizeof(Event) + ((len + 3u) & ~3u), at = *o.used;
    if (at > o.cap || rec > o.cap - at) { *o.overflow = 1u; return; }
    Event ev;
    ev.pos = (uint32_t)o.ch; ev.len = len; ev.kind = (uint16_t)kind; ev.pad = 0; ev.pad2 = 0;
    ev.first = first; ev.last = last;
    for (int k = 0; k < 8; k++) ev.v[k] = k < nv ? v[k] : 0;
    uint8_t *dst = o.arena + at;
    __builtin_memcpy(dst, &ev, sizeof(Event));                         // (records start on multiples of 4, not of 8)
    for (unsigned k = 0; k < ((len + 3u) & ~3u); k++) dst[sizeof(Event) + k] = k < len ? data[k] : 0;
    *o.used = at + rec;
    sm.stats[ST_EVENTS]++;
}

__device__ void message(FramesSmem &sm, const Emit &o, const unsigned char *text, int len, long long first, long long last)
{
    State &s = sm.st;
    s.grp_done = 1;
    for (int k = 0; k < TEXT_PAD; k++) s.msg[k] = k < len ? text[k] : 0;
    s.msg_len = len; s.msg_kind = s.grp_kind; s.msg_first = first; s.msg_last = last;
    sm.stats[ST_MESSAGES]++;
    if (s.grp_kind == KIND_EOM) sm.stats[ST_EOM]++;
    const int v[2] = {s.grp_kind, s.grp_n};
    emit(sm, o, NRSC5HIP_SAME_MESSAGE, first, last, v, 2, s.msg, (unsigned)len);
}

// a complete burst (sm.st.buf, len bytes, bits first .. last, preamble match at pre): the event, then the three-burst vote
__device__ void burst(FramesSmem &sm, const Emit &o, int kind, int len, long long pre, long long first, long long last)
{
    State &s = sm.st;
    sm.stats[ST_BURSTS]++;
    const bool joins = s.grp_n >= 1 && s.grp_n < 3 && kind == s.grp_kind && pre - s.grp_last <= VOTE_BITS;
    if (!joins) {
        if (s.grp_n > 0 && s.grp_done == 0) sm.stats[ST_NO_MESSAGE]++;  // the group it closes never agreed
        s.grp_n = 0; s.grp_done = 0; s.grp_kind = kind;
    }
    const int slot = s.grp_n;
    for (int k = 0; k < TEXT_PAD; k++) s.grp[slot][k] = k < len ? s.buf[k] : 0;
    s.grp_len[slot] = len; s.grp_n = slot + 1; s.grp_last = last;
    if (sm.burst_events) {
        const int v[3] = {kind, s.grp_n, (int)(first - pre)};
        emit(sm, o, NRSC5HIP_SAME_BURST, first, last, v, 3, s.buf, (unsigned)len);
    }
    if (s.grp_done) return;
    for (int j = 0; j < slot; j++) {                                    // byte for byte equal to an earlier burst of the group
        bool eq = s.grp_len[j] == len;
        for (int k = 0; k < len && eq; k++) eq = s.grp[j][k] == s.buf[k];
        if (eq) { message(sm, o, s.buf, len, first, last); return; }
    }
    if (s.grp_n == 3) {
        bool ok = s.grp_len[0] == len && s.grp_len[1] == len;
        for (int k = 0; k < len && ok; k++) {
            const unsigned char x = s.grp[0][k], y = s.grp[1][k], z = s.grp[2][k];
            if (x == y || x == z) s.buf[k] = x;
            else if (y == z) s.buf[k] = y;
            else ok = false;
        }
        if (ok) message(sm, o, s.buf, len, first, last);
        else { s.grp_done = 2; sm.stats[ST_NO_MESSAGE]++; }
    }
}

__device__ void one_bit(FramesSmem &sm, const Emit &o, unsigned bit, bool match)
{
    State &s = sm.st;
    const long long idx = s.nbits;
    s.nbits++;
    sm.stats[ST_BITS]++;
    s.reg = (s.reg >> 1 | bit << 15) & 0xFFFFu;
    if (s.state != MESSAGE && match && idx >= 15) {                     // sets the byte boundary
        if (s.state == SEARCH) { s.pre_bit = idx; sm.stats[ST_PREAMBLES]++; }
        s.state = PREAMBLE; s.fill = 0;
        return;
    }
    if (s.state == SEARCH) return;
    if (++s.fill < 8) return;
    s.fill = 0;
    const unsigned char byte = (unsigned char)(s.reg >> 8);
    if (s.state == PREAMBLE) {
        if (byte == 0xAB) return;
        if (byte == 'Z' || byte == 'N') { s.state = MESSAGE; s.len = 1; s.buf[0] = byte; s.first_bit = idx - 7; }
        else s.state = SEARCH;
        return;
    }
    bool abort = byte < 0x20 || byte > 0x7E;
    if (!abort) {
        s.buf[s.len++] = byte;
        if (s.len == 4) {
            const bool z = s.buf[0] == 'Z' && s.buf[1] == 'C' && s.buf[2] == 'Z' && s.buf[3] == 'C';
            const bool n = s.buf[0] == 'N' && s.buf[1] == 'N' && s.buf[2] == 'N' && s.buf[3] == 'N';
            if (n) { s.state = SEARCH; burst(sm, o, KIND_EOM, 4, s.pre_bit, s.first_bit, idx); return; }
            abort = !z;
        } else if (s.len > 4 && byte == '-') {                          // the third '-' behind the first '+'
            int plus = 0, dashes = 0;
            for (int k = 4; k < s.len; k++) {
                if (!plus) plus = s.buf[k] == '+';
                else dashes += s.buf[k] == '-';
            }
            if (dashes == 3) { s.state = SEARCH; burst(sm, o, KIND_HEADER, s.len, s.pre_bit, s.first_bit, idx); return; }
        }
        if (!abort && s.len >= TEXT_MAX) abort = true;
    }
    if (abort) { s.state = SEARCH; sm.stats[ST_ABORTED]++; }
}

__device__ void state_reset(FramesSmem &sm)
{
    unsigned *w = (unsigned *)&sm.st;
    for (unsigned k = 0; k < sizeof(State) / 4; k++) w[k] = 0;
    sm.st.msg_len = -1;
    for (int k = 0; k < NSTATS; k++)
        if (k != ST_SEAM_DROPS && k != ST_SEAM_INSERTS) sm.stats[k] = 0;                            // (those two are k_same_bits' own)
}

__global__ __launch_bounds__(64) void k_same_frames(FramesArgs a)
{
    __shared__ FramesSmem sm;
    const int wg = blockIdx.x, lane = threadIdx.x, ch = a.targets ? a.targets[wg] : wg;
    unsigned *stw = (unsigned *)&sm.st, *gw = (unsigned *)(a.state + ch);
    for (unsigned k = lane; k < sizeof(State) / 4; k += 64) stw[k] = gw[k];
    unsigned long long *gstats = a.stats + (long long)ch * NSTATS;
    for (int k = lane; k < NSTATS; k += 64) sm.stats[k] = gstats[k];
    if (lane == 0) sm.burst_events = a.burst_events;
    __syncthreads();
    const Emit o{a.arena + (size_t)ch * a.arena_cap, a.used + ch, a.overflow, a.arena_cap, ch};
    const int rst = a.reset_at ? a.reset_at[wg] : -1;
    int pos = 0;                                                       // bits of the call consumed
    for (int sg = 0; sg < a.nseg; sg++) {
        const uint8_t *bits = a.bits + (long long)wg * a.chan_stride + (long long)sg * a.seg_stride;
        const int n = a.counts[(long long)wg * a.nseg + sg];
        for (int base = 0; base < n; base += 64) {
            const int cn = min(64, n - base);
            // position-parallel: the 16 bits that end at base + lane, the 15 in front of the chunk from the register (its bit 15 is the newest)
            if (lane < 15) sm.win[lane] = (uint8_t)(sm.st.reg >> (lane + 1) & 1u);
            sm.win[15 + lane] = lane < cn ? (uint8_t)(bits[base + lane] & 1u) : (uint8_t)0;
            __syncthreads();
            unsigned v = 0;
            for (int k = 0; k < 16; k++) v |= (unsigned)sm.win[lane + k] << k;
            sm.match[lane] = v == 0xABABu;
            __syncthreads();
            if (lane == 0) {
                for (int i = 0; i < cn; i++) {
                    if (pos + i == rst) state_reset(sm);
                    one_bit(sm, o, sm.win[15 + i], sm.match[i] != 0);
                }
            }
            pos += cn;
            __syncthreads();
        }
    }
    if (lane == 0 && pos == rst) state_reset(sm);
    __syncthreads();
    for (unsigned k = lane; k < sizeof(State) / 4; k += 64) gw[k] = stw[k];
    for (int k = lane; k < NSTATS; k += 64)
        if (k != ST_SEAM_DROPS && k != ST_SEAM_INSERTS) gstats[k] = sm.stats[k];
}

__global__ __launch_bounds__(256) void k_same_keep(KeepArgs a)
{
    const int ch = blockIdx.y;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (long long)gridDim.x * blockDim.x)
        a.c_new[ch * a.c_stride + i] = a.c_old[ch * a.c_stride + i + a.shift];
}

}  // namespace

void launch_tones(hipStream_t s, int tiles, int nchan, const TonesArgs &a)
{
    fm::count_launch();
    hipLaunchKernelGGL(k_same_tones, dim3(tiles, nchan), dim3(64), 0, s, a);
}

void launch_bits(hipStream_t s, int nchan, const BitsArgs &a)
{
    fm::count_launch();
    hipLaunchKernelGGL(k_same_bits, dim3(a.nwin, nchan), dim3(64), 0, s, a);
}

void launch_frames(hipStream_t s, int nwg, const FramesArgs &a)
{
    fm::count_launch();
    hipLaunchKernelGGL(k_same_frames, dim3(nwg), dim3(64), 0, s, a);
}

void launch_keep(hipStream_t s, int nchan, const KeepArgs &a)
{
    fm::count_launch();
    long long blocks = (a.count + 255) / 256;
    if (blocks > 16) blocks = 16;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_same_keep, dim3((unsigned)blocks, nchan), dim3(256), 0, s, a);
}

}  // namespace same
}  // namespace nrsc5
