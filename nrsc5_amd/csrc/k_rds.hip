// RDS / RBDS of a station's analog host from the discriminator output d[m] at Fs1 = 372 093.75 S/s (include/nrsc5hip.h, "RDS"; the definition:
// DESIGN.md (p)).  Every quantity is a function of absolute sample indices, no recurrence in the signal path: any chunking gives the same bits,
// events and counters.
//   k_rds_mf      one workgroup = MT = 64 consecutive grid points of one channel (8 per bit, point r at 11907 r / 304 samples).  The d span is
//                 mixed with the exact 57 kHz phasor ((1824 m) mod 11907 indexes the pilot's table) and staged in LDS as float2; the block's
//                 4 waves each sum a quarter of the 1255 taps of the 64 points, lane = point, and wave 0 adds the quarters in order.  The
//                 table is tap-major and indexed by r mod 304 (51 r mod 304, the phase, is a bijection of it): the 64 lanes of one tap read
//                 64 neighbouring floats.
//   k_rds_bits    one wave = one complete window of 152 bits: the 8 timing energies (19 terms per lane in order, then a butterfly), s_w, the
//                 seam rule against s_{w-1} (kept from the last call, or summed again from the y of window w - 1), and up to 153 decisions
//                 Re(y[r_i] conj y[r_{i-1}]) < 0.
//   k_rds_groups  one wave = one channel.  Per 64 bits a position-parallel phase (lane = bit position: the syndrome of the 26 bits that end
//                 there, which names the offset word it is valid with) and an in-order phase on lane 0 (sync, blocks, groups, content; the
//                 state lives in HBM and is held in LDS for the launch).  Events go to the channel's arena, sized by the host from the bits.
//   k_rds_keep    the y of the incomplete window (and the 8 points in front of it) move to the front of the other buffer.
#include <hip/hip_runtime.h>
#include "fm_audio.h"

namespace nrsc5 {
namespace rds {
namespace {

__device__ __forceinline__ long long grid_floor(long long r) { return ((long long)DEN * r) / GRID; }

__global__ __launch_bounds__(256) void k_rds_mf(MfArgs a)
{
    HIP_DYNAMIC_SHARED(float2, sm);
    float2 *vs = sm, *part = sm + MF_SPAN;                    // part: [4][MT]
    const int ch = blockIdx.y, tid = threadIdx.x, lane = tid & 63, qtr = tid >> 6;
    const long long rt0 = a.r0 + (long long)blockIdx.x * MT;
    const long long left = a.r0 + a.r_count - rt0;
    const int cnt = left < MT ? (int)left : MT;
    if (cnt <= 0) return;
    const long long m_lo = grid_floor(rt0) - HALF;            // vs[k] = v[m_lo + k]
    const int span = (int)(grid_floor(rt0 + cnt - 1) - grid_floor(rt0)) + NT;
    const float *d = a.d + (long long)ch * a.d_stride;
    for (int k = tid; k < span; k += 256) {
        const long long m = m_lo + k;
        float2 v = make_float2(0.0f, 0.0f);
        if (m >= 0) {                                         // samples in front of the stream are zero
            const float2 t = a.cs[(int)(((long long)SC_NUM * m) % DEN)];
            const float x = d[m - a.d_base];
            v = make_float2(x * t.x, -(x * t.y));             // d exp(-j phi57)
        }
        vs[k] = v;
    }
    __syncthreads();
    float re = 0.0f, im = 0.0f;
    if (lane < cnt) {
        const long long r = rt0 + lane;
        const float2 *v = vs + (int)(grid_floor(r) - HALF - m_lo);
        const float *tab = a.tab + (int)(r % GRID);
        const int tq = (NT + 3) / 4, j0 = qtr * tq, j1 = min(NT, j0 + tq);
        for (int j = j0; j < j1; j++) {
            const float t = tab[j * GRID];
            const float2 x = v[j];
            re = fmaf(t, x.x, re); im = fmaf(t, x.y, im);
        }
    }
    part[qtr * MT + lane] = make_float2(re, im);
    __syncthreads();
    if (tid < cnt) {
        float2 s = part[tid];
        for (int q = 1; q < 4; q++) { s.x += part[q * MT + tid].x; s.y += part[q * MT + tid].y; }
        a.y[(long long)ch * a.y_stride + (rt0 + tid - a.y_base)] = s;
    }
}

// the 8 timing energies of the window that starts at y0, lane 8 g + s: bits g, g + 8, .. in order, then a butterfly over g -> argmax, ties to the lowest s
__device__ __forceinline__ int window_timing(const float2 *y0, int lane, float *energy)
{
    const int s = lane & 7, g = lane >> 3;
    float e = 0.0f;
    for (int k = 0; k < WIN_BITS / 8; k++) {
        const float2 v = y0[S * (g + 8 * k) + s];
        e += v.x * v.x + v.y * v.y;
    }
    for (int st = 8; st <= 32; st <<= 1) e += __shfl_xor(e, st);
    int best = 0;
    float eb = __shfl(e, 0);
    for (int q = 1; q < S; q++) {
        const float eq = __shfl(e, q);
        if (eq > eb) { eb = eq; best = q; }
    }
    *energy = e;
    return best;
}

__global__ __launch_bounds__(64) void k_rds_bits(BitsArgs a)
{
    const int ch = blockIdx.y, wi = blockIdx.x, lane = threadIdx.x;
    const long long w = a.w0 + wi;
    const float2 *y = a.y + (long long)ch * a.y_stride - a.y_base;     // y[r] by its absolute index
    float e;
    const int sw = window_timing(y + w * WIN_PTS, lane, &e);
    int sp = -1;
    if (w > 0) {
        if (wi > 0) { float ep; sp = window_timing(y + (w - 1) * WIN_PTS, lane, &ep); }
        else sp = a.s_in[ch];
    }
    const long long first = w * WIN_PTS + sw;
    // the window's sampling points Q[0 ..): an inserted point, or the first one dropped, by the gap to the last point of window w - 1
    long long q0 = first, lastp = 0;
    int nq = WIN_BITS, ins = 0, drop = 0;
    if (w > 0) {
        const int gap = S + sw - sp;
        lastp = w * WIN_PTS - S + sp;
        if (gap < 4) { q0 = first + S; nq = WIN_BITS - 1; drop = 1; }
        else if (gap > 12) { nq = WIN_BITS + 1; ins = 1; }
    }
    const int nb = w > 0 ? nq : nq - 1;                                // the first point of a session has no predecessor
    uint8_t *bits = a.bits + ((long long)ch * a.nwin + wi) * BITS_STRIDE;
    for (int b = lane; b < BITS_STRIDE; b += 64) {
        uint8_t bit = 0;
        if (b < nb) {
            const int qi = w > 0 ? b : b + 1;                          // index in Q of the bit's own point
            long long rc, rp;
            if (ins) {
                rc = qi == 0 ? lastp + S : first + (long long)S * (qi - 1);
                rp = qi == 0 ? lastp : (qi == 1 ? lastp + S : first + (long long)S * (qi - 2));
            } else {
                rc = q0 + (long long)S * qi;
                rp = qi == 0 ? lastp : q0 + (long long)S * (qi - 1);
            }
            const float2 c = y[rc], p = y[rp];
            bit = (c.x * p.x + c.y * p.y) < 0.0f ? 1 : 0;
        }
        bits[b] = bit;
    }
    if (lane < S) {
        if (a.energy) a.energy[((long long)ch * a.nwin + wi) * S + lane] = e;
    }
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

// ------------------------------------------------------------------------------------------------------------------ blocks, groups, content
constexpr unsigned POLY = 0x5B9;                                       // x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
constexpr int NERR = 26 + 25;                                          // single bits, two neighbouring bits

struct GroupsSmem {
    State st;
    unsigned long long stats[NSTATS];
    unsigned short bit_syn[26];                                        // syndrome of bit k of a 26-bit word
    unsigned short err_syn[NERR];
    unsigned err_mask[NERR];
    unsigned short syn[64];
    uint8_t win[64 + 25];
};

__device__ __forceinline__ unsigned syndrome_of(unsigned word)
{
    for (int k = 25; k >= 10; k--)
        if (word >> k & 1u) word ^= POLY << (k - 10);
    return word & 0x3FFu;
}

__device__ __forceinline__ int offset_class(unsigned syn)
{
    return syn == 0x0FCu ? 0 : syn == 0x198u ? 1 : (syn == 0x168u || syn == 0x350u) ? 2 : syn == 0x1B4u ? 3 : -1;
}

struct Emit {                                                           // lane 0's view of the channel's arena
    uint8_t *arena; unsigned *used, *overflow; unsigned cap; int ch;
};

__device__ void emit(GroupsSmem &sm, const Emit &o, int kind, const int *v, int nv, const unsigned char *data, unsigned len)
{
    const unsigned rec = (unsigned)sizeof(Event) + ((len + 3u) & ~3u), at = *o.used;
    if (at > o.cap || rec > o.cap - at) { *o.overflow = 1u; return; }
    Event ev;
    ev.pos = (uint32_t)o.ch; ev.len = len; ev.kind = (uint16_t)kind; ev.pad = 0; ev.pad2 = 0;
    ev.group = sm.st.gindex; ev.bit = sm.st.nbits - 1;
    for (int k = 0; k < 8; k++) ev.v[k] = k < nv ? v[k] : 0;
    uint8_t *dst = o.arena + at;
    __builtin_memcpy(dst, &ev, sizeof(Event));                         // (records start on multiples of 4, not of 8)
    for (unsigned k = 0; k < ((len + 3u) & ~3u); k++) dst[sizeof(Event) + k] = k < len ? data[k] : 0;
    *o.used = at + rec;
    sm.stats[ST_EVENTS]++;
}

__device__ void set_pi(GroupsSmem &sm, const Emit &o, int v)
{
    State &s = sm.st;
    if (v == s.pi) return;
    s.pi = v;
    s.ps_mask = 0; s.ps_have = 0;
    s.rt_mask = 0; s.rt_ab = -1; s.rt_ver = -1; s.rt_have = 0; s.rt_last_len = -1;
    emit(sm, o, NRSC5HIP_RDS_PI, &v, 1, nullptr, 0);
}

__device__ void group(GroupsSmem &sm, const Emit &o, int raw)
{
    State &s = sm.st;
    const int a = s.gw[0], b = s.gw[1], c = s.gw[2], d = s.gw[3];
    const int gt = b >> 12, ver = b >> 11 & 1;
    sm.stats[ST_GROUPS]++;
    sm.stats[ST_TYPE0 + 2 * gt + ver]++;
    if (raw) emit(sm, o, NRSC5HIP_RDS_GROUP, s.gw, 4, nullptr, 0);
    set_pi(sm, o, a);
    if (ver) set_pi(sm, o, c);
    s.pty = b >> 5 & 31; s.tp = b >> 10 & 1;
    if (gt == 0) {
        const int seg = b & 3;
        s.ta = b >> 4 & 1; s.ms = b >> 3 & 1;
        s.di = (s.di & ~(1 << (3 - seg))) | (b >> 2 & 1) << (3 - seg);
        s.ps_buf[2 * seg] = (unsigned char)(d >> 8); s.ps_buf[2 * seg + 1] = (unsigned char)(d & 255);
        s.ps_mask |= 1 << seg;
        if (s.ps_mask == 15) {
            bool same = s.ps_have != 0;
            for (int k = 0; k < 8 && same; k++) same = s.ps_buf[k] == s.ps_last[k];
            if (!same) {
                for (int k = 0; k < 8; k++) s.ps_last[k] = s.ps_buf[k];
                s.ps_have = 1;
                emit(sm, o, NRSC5HIP_RDS_PS, &s.pi, 1, s.ps_last, 8);
            }
        }
    } else if (gt == 2) {
        const int flag = b >> 4 & 1, seg = b & 15, per = ver ? 2 : 4;
        if (flag != s.rt_ab || ver != s.rt_ver) {
            for (int k = 0; k < 64; k++) s.rt_buf[k] = 0;
            s.rt_mask = 0; s.rt_ab = flag; s.rt_ver = ver;
        }
        unsigned char *q = s.rt_buf + per * seg;
        if (ver) { q[0] = (unsigned char)(d >> 8); q[1] = (unsigned char)(d & 255); }
        else { q[0] = (unsigned char)(c >> 8); q[1] = (unsigned char)(c & 255); q[2] = (unsigned char)(d >> 8); q[3] = (unsigned char)(d & 255); }
        s.rt_mask |= 1 << seg;
        int length = 0;
        for (int sg = 0; sg < 16; sg++) {
            if (!(s.rt_mask >> sg & 1)) break;
            bool cr = false;
            for (int k = 0; k < per; k++) cr = cr || s.rt_buf[per * sg + k] == 0x0D;
            if (cr || sg == 15) { length = sg + 1; break; }
        }
        if (length) {
            const int n = per * length;
            bool same = s.rt_have != 0 && s.rt_last_len == n;
            for (int k = 0; k < n && same; k++) same = s.rt_buf[k] == s.rt_last[k];
            if (!same) {
                for (int k = 0; k < 64; k++) s.rt_last[k] = k < n ? s.rt_buf[k] : 0;
                s.rt_have = 1; s.rt_last_len = n;
                const int v[2] = {s.pi, flag};
                emit(sm, o, NRSC5HIP_RDS_RT, v, 2, s.rt_last, (unsigned)n);
            }
        }
    } else if (gt == 4 && ver == 0) {
        const int off = d & 31;
        const int v[4] = {(b & 3) << 15 | c >> 1, (c & 1) << 4 | d >> 12, d >> 6 & 63, (d >> 5 & 1) ? -off : off};
        if (!s.clk_have || v[0] != s.clk[0] || v[1] != s.clk[1] || v[2] != s.clk[2] || v[3] != s.clk[3]) {
            s.clk_have = 1;
            for (int k = 0; k < 4; k++) s.clk[k] = v[k];
            emit(sm, o, NRSC5HIP_RDS_CLOCK, v, 4, nullptr, 0);
        }
    }
}

__device__ void block(GroupsSmem &sm, const Emit &o, int cls, unsigned reg, unsigned syn, int raw, int burst)
{
    State &s = sm.st;
    const unsigned off0 = cls == 0 ? 0x0FCu : cls == 1 ? 0x198u : cls == 2 ? 0x168u : 0x1B4u, off1 = cls == 2 ? 0x350u : off0;
    bool ok = syn == off0 || syn == off1;
    unsigned word = reg >> 10;
    if (ok) { sm.stats[ST_VALID]++; s.bad_run = 0; }
    else {
        const int nerr = burst >= 2 ? NERR : burst == 1 ? 26 : 0;
        for (int t = 0; t < 2 && !ok; t++) {
            if (t == 1 && off1 == off0) break;
            const unsigned e = syn ^ (t ? off1 : off0);
            for (int k = 0; k < nerr; k++)
                if (sm.err_syn[k] == e) { ok = true; word = (reg ^ sm.err_mask[k]) >> 10; break; }
        }
        sm.stats[ok ? ST_CORRECTED : ST_INVALID]++;
        if (!ok) s.bad_run++;                                          // a corrected block neither counts nor ends the run
    }
    if (cls == 0) { s.in_group = 1; s.gmask = 0; s.gindex = s.ngroups; s.ngroups++; }
    if (s.in_group && ok) { s.gw[cls] = (int)word; s.gmask |= 1 << cls; }
    if (cls == 3 && s.in_group) {
        s.in_group = 0;
        if (s.gmask == 15) group(sm, o, raw);
        else sm.stats[ST_DROPPED]++;
    }
    if (s.bad_run >= LOSS_BLOCKS) {
        s.synced = 0; s.in_group = 0;
        sm.stats[ST_LOST]++;
        for (int k = 0; k < 26; k++) s.ring[k] = 255 << 8;
    }
}

__device__ void one_bit(GroupsSmem &sm, const Emit &o, unsigned bit, unsigned syn, int raw, int burst)
{
    State &s = sm.st;
    const long long idx = s.nbits;
    s.nbits++;
    sm.stats[ST_BITS]++;
    s.reg = (s.reg << 1 | bit) & 0x3FFFFFFu;
    if (!s.synced) {
        const int cls = idx >= 25 ? offset_class(syn) : -1;
        const int slot = (int)(idx % 26);
        int run = 0;
        if (cls >= 0) {
            const int pc = s.ring[slot] >> 8, pr = s.ring[slot] & 255;
            run = (pr > 0 && pc == ((cls + 3) & 3)) ? pr + 1 : 1;
        }
        s.ring[slot] = (cls < 0 ? 255 : cls) << 8 | run;
        if (run >= 3) {
            s.synced = 1;
            sm.stats[ST_GAINED]++;
            s.exp = (cls + 1) & 3; s.fill = 0; s.bad_run = 0; s.in_group = 0;
            for (int k = 0; k < 26; k++) s.ring[k] = 255 << 8;
        }
        return;
    }
    if (++s.fill == 26) {
        s.fill = 0;
        block(sm, o, s.exp, s.reg, syn, raw, burst);
        s.exp = (s.exp + 1) & 3;
    }
}

__device__ void state_reset(GroupsSmem &sm)
{
    State &s = sm.st;
    unsigned *w = (unsigned *)&s;
    for (unsigned k = 0; k < sizeof(State) / 4; k++) w[k] = 0;
    for (int k = 0; k < 26; k++) s.ring[k] = 255 << 8;
    s.pi = -1; s.rt_ab = -1; s.rt_ver = -1; s.rt_last_len = -1;
    for (int k = 0; k < NSTATS; k++)
        if (k != ST_SEAM_DROPS && k != ST_SEAM_INSERTS) sm.stats[k] = 0;                            // (those two are k_rds_bits' own)
}

__global__ __launch_bounds__(64) void k_rds_groups(GroupsArgs a)
{
    __shared__ GroupsSmem sm;
    const int wg = blockIdx.x, lane = threadIdx.x, ch = a.targets ? a.targets[wg] : wg;
    unsigned *stw = (unsigned *)&sm.st, *gw = (unsigned *)(a.state + ch);
    for (unsigned k = lane; k < sizeof(State) / 4; k += 64) stw[k] = gw[k];
    unsigned long long *gstats = a.stats + (long long)ch * NSTATS;
    for (int k = lane; k < NSTATS; k += 64) sm.stats[k] = gstats[k];
    if (lane < 26) sm.bit_syn[lane] = (unsigned short)syndrome_of(1u << lane);
    if (lane < NERR) {
        const unsigned mk = lane < 26 ? 1u << lane : 3u << (lane - 26);
        sm.err_mask[lane] = mk; sm.err_syn[lane] = (unsigned short)syndrome_of(mk);
    }
    __syncthreads();
    const Emit o{a.arena + (size_t)ch * a.arena_cap, a.used + ch, a.overflow, a.arena_cap, ch};
    const int rst = a.reset_at ? a.reset_at[wg] : -1;
    int pos = 0;                                                       // bits of the call consumed
    for (int sg = 0; sg < a.nseg; sg++) {
        const uint8_t *bits = a.bits + (long long)wg * a.chan_stride + (long long)sg * a.seg_stride;
        const int n = a.counts[(long long)wg * a.nseg + sg];
        for (int base = 0; base < n; base += 64) {
            const int cn = min(64, n - base);
            // position-parallel: the 26 bits that end at base + lane, the 25 in front of the chunk from the register
            if (lane < 25) sm.win[lane] = (uint8_t)(sm.st.reg >> (24 - lane) & 1u);
            sm.win[25 + lane] = lane < cn ? (uint8_t)(bits[base + lane] & 1u) : (uint8_t)0;
            __syncthreads();
            unsigned syn = 0;
            for (int k = 0; k < 26; k++)
                if (sm.win[lane + k]) syn ^= sm.bit_syn[25 - k];
            sm.syn[lane] = (unsigned short)syn;
            __syncthreads();
            if (lane == 0) {
                for (int i = 0; i < cn; i++) {
                    if (pos + i == rst) state_reset(sm);
                    one_bit(sm, o, sm.win[25 + i], sm.syn[i], a.raw, a.burst);
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

__global__ __launch_bounds__(256) void k_rds_keep(KeepArgs a)
{
    const int ch = blockIdx.y;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (long long)gridDim.x * blockDim.x)
        a.y_new[ch * a.y_stride + i] = a.y_old[ch * a.y_stride + i + a.shift];
}

}  // namespace

void launch_mf(hipStream_t s, int tiles, int nchan, const MfArgs &a)
{
    fm::count_launch();
    hipLaunchKernelGGL(k_rds_mf, dim3(tiles, nchan), dim3(256), sizeof(float2) * (MF_SPAN + 4 * MT), s, a);
}

void launch_bits(hipStream_t s, int nchan, const BitsArgs &a)
{
    fm::count_launch();
    hipLaunchKernelGGL(k_rds_bits, dim3(a.nwin, nchan), dim3(64), 0, s, a);
}

void launch_groups(hipStream_t s, int nwg, const GroupsArgs &a)
{
    fm::count_launch();
    hipLaunchKernelGGL(k_rds_groups, dim3(nwg), dim3(64), 0, s, a);
}

void launch_keep(hipStream_t s, int nchan, const KeepArgs &a)
{
    fm::count_launch();
    long long blocks = (a.count + 255) / 256;
    if (blocks > 16) blocks = 16;
    hipLaunchKernelGGL(k_rds_keep, dim3((unsigned)blocks, nchan), dim3(256), 0, s, a);
}

}  // namespace rds
}  // namespace nrsc5
