// K=9 rate-1/3 tail-biting Viterbi of the AM path (conv_dec.c:402-453, conv_gen.h:32-123; nrsc5_conv_decode_e1 / _e2_e3,
// decode.c:47-61), device-inline: the 256-work-item form, the one-wave form, the same decode in segment waves with their checking
// waves, and the re-encode bit-error count.  The kernels that use it: k_am.hip (PIDS, inside the block step) and k_am_decode.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "nrsc5_dev.h"
#include "wave_ops.h"

namespace nrsc5 {

// =====================================================================================================
// K=9 rate-1/3 tail-biting Viterbi, 256 states = 256 work-items (conv_dec.c:402-453, conv_gen.h:32-123)
// =====================================================================================================
// Work-item n owns new state n: predecessors 2b, 2b+1 with b = n & 127, branch metric +m for n < 128 and -m above
// (acs_butterfly).  int32 metrics, no normalisation (inputs are +-1/0: |metric| <= 3 per step); ties pick
// predecessor 2b+1 as `if (sum0 > sum1)` does.  Decisions: one ballot per wave and step (4 x u64 per step).
struct K9Smem {
    int metric[2][256];
    int8_t soft[3 * 256];
    unsigned long long chunk[4 * 256];
    int red_val[4], red_idx[4];
    int state;
};

__device__ inline void viterbi_k9_block(const int8_t *coded, int len, unsigned g0, unsigned g1, unsigned g2,
                                        unsigned long long *dec, uint32_t *out, K9Smem &sm)
{
    const int n = threadIdx.x, b = n & 127;
    const unsigned reg = ((unsigned)b << 1) & 0xfeu;           // gen_state_info, conv_dec.c:137-153
    const int flip = n >= 128 ? -1 : 1;
    const int sg0 = flip * ((__popc(reg & g0) & 1) ? 1 : -1);
    const int sg1 = flip * ((__popc(reg & g1) & 1) ? 1 : -1);
    const int sg2 = flip * ((__popc(reg & g2) & 1) ? 1 : -1);
    const int steps = len + 2 * VIT_EXTRA, j0 = len - VIT_EXTRA;
    int cur = 0;
    sm.metric[0][n] = 0;                                       // reset_decoder: all-zero for tail biting
    for (int t0 = 0; t0 < steps; t0 += 256) {
        __syncthreads();
        if (t0 + n < steps) {
            const int j = (j0 + t0 + n) % len;
            sm.soft[3 * n] = coded[3 * j]; sm.soft[3 * n + 1] = coded[3 * j + 1]; sm.soft[3 * n + 2] = coded[3 * j + 2];
        }
        __syncthreads();
        const int nst = min(256, steps - t0);
        for (int s = 0; s < nst; s++) {
            const int m = sm.soft[3 * s] * sg0 + sm.soft[3 * s + 1] * sg1 + sm.soft[3 * s + 2] * sg2;
            const int e = sm.metric[cur][2 * b], o = sm.metric[cur][2 * b + 1];
            const int pa = e + m, pc = o - m;
            const bool take_e = pa > pc;
            sm.metric[cur ^ 1][n] = take_e ? pa : pc;
            const unsigned long long w = __ballot(!take_e);    // bit = 1: survivor came from 2b+1
            if ((n & 63) == 0) dec[(size_t)(t0 + s) * 4 + (n >> 6)] = w;
            cur ^= 1;
            __syncthreads();
        }
    }
    // end state: first maximum in state order (conv_dec.c:310-318)
    {
        int v = sm.metric[cur][n], idx = n;
        for (int m = 32; m >= 1; m >>= 1) {
            const int ov = __shfl_xor(v, m), oi = __shfl_xor(idx, m);
            if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
        }
        if ((n & 63) == 0) { sm.red_val[n >> 6] = v; sm.red_idx[n >> 6] = idx; }
        __threadfence_block();
        __syncthreads();
        if (n == 0) {
            for (int w = 1; w < 4; w++) if (sm.red_val[w] > v) { v = sm.red_val[w]; idx = sm.red_idx[w]; }
            sm.state = idx;
        }
    }
    // traceback: decisions staged through LDS 256 steps at a time, walked by one work-item
    const int nchunks = (steps + 255) / 256;
    uint32_t accw = 0; int accidx = -1;
    for (int c = nchunks - 1; c >= 0; c--) {
        const int t0 = c * 256, nst = min(256, steps - t0);
        __syncthreads();
        for (int k = n; k < 4 * nst; k += 256) sm.chunk[k] = dec[(size_t)t0 * 4 + k];
        __syncthreads();
        if (n == 0) {
            unsigned state = (unsigned)sm.state;
            for (int s = nst - 1; s >= 0; s--) {
                const int t = t0 + s;
                const unsigned bit = (unsigned)(sm.chunk[4 * s + (state >> 6)] >> (state & 63)) & 1u;
                if (t >= VIT_EXTRA && t < len + VIT_EXTRA) {
                    const int i = t - VIT_EXTRA;
                    if ((i >> 5) != accidx) { if (accidx >= 0) out[accidx] = accw; accidx = i >> 5; accw = 0; }
                    accw |= ((state >> 7) & 1u) << (i & 31);   // vals[state]: the newest input bit
                }
                state = ((state << 1) & 0xfeu) | bit;           // vstate_lshift
            }
            sm.state = (int)state;
        }
    }
    if (n == 0 && accidx >= 0) out[accidx] = accw;
    __threadfence_block();
    __syncthreads();
}

// ---- the same trellis on ONE wave64, two steps per LDS round trip ------------------------------------------------------
// Lane L reads old states 4L..4L+3 (one 16-byte LDS read).  Step t: butterflies 2L and 2L+1 give the four intermediate
// states (i0 << 7) | (2L + xh); step t+1: butterflies L and L + 64 combine them into the four new states
// (i1 << 7) | (i0 << 6) | L, written at stride 64 (conflict-free) into the other half of a ping-pong buffer, where they are
// again states 4L'..4L'+3 of some lane L'.  Same eight compares per lane as two single steps, same tie rule, same int32
// metrics -> bit-identical decisions; half the LDS latency and loop overhead per trellis step.
// No workgroup barrier: a single-wave workgroup orders its own LDS traffic (WAVE_LDS_SYNC, wave_ops.h).
// Decisions per step pair: one byte per lane -- bit i0 * 2 + xh for step t (1 = survivor from old state 4L + 2 xh + 1),
// bit 4 + i1 * 2 + i0 for step t+1 (1 = survivor from xh = 1) -- so a step pair of the traceback needs ONE byte, the one
// of lane n & 63: prev = ((n & 63) << 2) | xh << 1 | xl, read at a wave-uniform address from a chunk staged in LDS.
struct K9WSmem { int metric[2][256]; };   // 2 KB per frame in flight (the traceback stages decisions in the same 2 KB): 32 decode
                                         // workgroups per CU still leave room for k_am_block's 70 KB tile

__device__ inline int k9_sign_word(unsigned b, unsigned g0, unsigned g1, unsigned g2)
{
    const unsigned reg = (b << 1) & 0xfeu;
    const int s0 = (__popc(reg & g0) & 1) ? 1 : -1, s1 = (__popc(reg & g1) & 1) ? 1 : -1, s2 = (__popc(reg & g2) & 1) ? 1 : -1;
    return (s0 & 0xff) | ((s1 & 0xff) << 8) | ((s2 & 0xff) << 16);
}

__device__ inline int k9_soft_word(const int8_t *coded, int j)
{
    return (coded[3 * j] & 0xff) | ((coded[3 * j + 1] & 0xff) << 8) | ((coded[3 * j + 2] & 0xff) << 16);
}

struct K9Signs { int a, b, c, d; };
__device__ inline K9Signs k9_signs(int lane, unsigned g0, unsigned g1, unsigned g2)
{
    K9Signs sg;
    sg.a = k9_sign_word(2u * lane, g0, g1, g2); sg.b = k9_sign_word(2u * lane + 1u, g0, g1, g2);             // step t: b = 2L + xh
    sg.c = k9_sign_word((unsigned)lane, g0, g1, g2); sg.d = k9_sign_word((unsigned)lane + 64u, g0, g1, g2);   // step t+1: b = (i0 << 6) | L
    return sg;
}

// A frame is steps = len + 2 * VIT_EXTRA trellis steps (even for every frame length of the AM path) = npairs step pairs, walked
// forward in chunks of 64 step pairs and backward in chunks of 32.
__host__ __device__ inline int k9_pairs(int len) { return (len + 2 * VIT_EXTRA) >> 1; }
__host__ __device__ inline int k9_chunks(int len) { return (k9_pairs(len) + 63) >> 6; }

// Forward pass over the chunks [c0, c1): the metrics are in sm.metric[0] on entry (every chunk but the frame's last is an even
// number of step pairs, so a chunk boundary always finds them there); returns the half that holds them after the last pair.
// Decisions are written for chunks >= cstore only (a segment wave's warm-up chunks belong to its predecessor), and the metrics
// the wave enters chunk `cstore` with go to `snap` (k9_forward_fix checks them against the predecessor's end metrics).
__device__ inline int k9_forward_chunks(const int8_t *coded, int len, const K9Signs &sg, unsigned long long *dec, K9WSmem &sm,
                                        int c0, int c1, int cstore, int *snap)
{
    const int lane = threadIdx.x & 63;
    const int j0 = len - VIT_EXTRA, npairs = k9_pairs(len);
    int cur = 0;
    for (int c = c0; c < c1; c++) {
        const int p0 = c << 6, np = min(64, npairs - p0);
        if (snap && c == cstore) *(int4 *)&snap[4 * lane] = *(const int4 *)&sm.metric[cur][4 * lane];
        const bool store = c >= cstore;                        // wave-uniform
        int aw0 = 0, aw1 = 0;                                   // this lane's step pair of the chunk
        if (lane < np) {
            const int t = 2 * (p0 + lane);
            aw0 = k9_soft_word(coded, (j0 + t) % len);
            aw1 = k9_soft_word(coded, (j0 + t + 1) % len);
        }
        for (int s = 0; s < np; s++) {
            const int a0 = wave_readlane(aw0, s), a1 = wave_readlane(aw1, s);
            const int mA = dot4_i8(a0, sg.a, 0), mB = dot4_i8(a0, sg.b, 0), nC = dot4_i8(a1, sg.c, 0), nD = dot4_i8(a1, sg.d, 0);
            const int4 old = *(const int4 *)&sm.metric[cur][4 * lane];
            // step t
            const int e00 = old.x + mA, o00 = old.y - mA, e10 = old.x - mA, o10 = old.y + mA;   // xh = 0: i0 = 0, i0 = 1
            const int e01 = old.z + mB, o01 = old.w - mB, e11 = old.z - mB, o11 = old.w + mB;   // xh = 1
            const bool t00 = e00 > o00, t01 = e01 > o01, t10 = e10 > o10, t11 = e11 > o11;       // t[i0][xh]: survivor from the even predecessor
            const int u00 = t00 ? e00 : o00, u01 = t01 ? e01 : o01, u10 = t10 ? e10 : o10, u11 = t11 ? e11 : o11;
            // step t+1: new state (i1, i0, L) from u[i0][0] (even) and u[i0][1] (odd)
            const int f00 = u00 + nC, p00 = u01 - nC, f10 = u00 - nC, p10 = u01 + nC;           // i0 = 0: i1 = 0, i1 = 1
            const int f01 = u10 + nD, p01 = u11 - nD, f11 = u10 - nD, p11 = u11 + nD;           // i0 = 1
            const bool r00 = f00 > p00, r01 = f01 > p01, r10 = f10 > p10, r11 = f11 > p11;       // r[i1][i0]
            int *nxt = sm.metric[cur ^ 1];
            nxt[lane] = r00 ? f00 : p00;                        // state (0, 0, L)
            nxt[64 + lane] = r01 ? f01 : p01;                   // state (0, 1, L)
            nxt[128 + lane] = r10 ? f10 : p10;                  // state (1, 0, L)
            nxt[192 + lane] = r11 ? f11 : p11;                  // state (1, 1, L)
            // this lane's eight decisions of the step pair in one byte: bit i0*2+xh for step t, bit 4+i1*2+i0 for step t+1
            const unsigned dbyte = (t00 ? 0u : 1u) | (t01 ? 0u : 2u) | (t10 ? 0u : 4u) | (t11 ? 0u : 8u)
                                 | (r00 ? 0u : 16u) | (r01 ? 0u : 32u) | (r10 ? 0u : 64u) | (r11 ? 0u : 128u);
            if (store) ((uint8_t *)dec)[(size_t)(p0 + s) * 64 + lane] = (uint8_t)dbyte;     // one 64-byte row per step pair, fire and forget
            cur ^= 1;
            WAVE_LDS_SYNC();
        }
    }
    return cur;
}

// end state: first maximum in state order (conv_dec.c:310-318); m = this lane's metrics of states 4L .. 4L+3
__device__ inline unsigned k9_end_state(int4 m)
{
    const int lane = threadIdx.x & 63;
    int v = m.x, idx = 4 * lane;
    if (m.y > v) { v = m.y; idx = 4 * lane + 1; }
    if (m.z > v) { v = m.z; idx = 4 * lane + 2; }
    if (m.w > v) { v = m.w; idx = 4 * lane + 3; }
    for (int k = 32; k >= 1; k >>= 1) {
        const int ov = __shfl_xor(v, k), oi = __shfl_xor(idx, k);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    return (unsigned)wave_uniform(idx);
}

// Traceback over the 32-pair chunks c_hi - 1 .. c_lo (downwards) from `state`, two steps per iteration; a chunk's decisions are
// staged in LDS (the metrics are dead: 2 KB = 32 step pairs) and looked up at a wave-uniform address.  Output words are written for
// chunks < c_out only (the chunks above are a segment wave's run-in); `arrive` = the state on entering chunk c_out - 1.
// Chunk c holds steps 64 c .. 64 c + 63 = frame bits 64 c - 32 .. 64 c + 31: words 2c - 1 (low half) and 2c (high half), and no
// other chunk writes those words.
__device__ inline unsigned k9_traceback_chunks(const unsigned long long *dec, int len, K9WSmem &sm, unsigned state, int c_hi, int c_lo, int c_out,
                                               uint32_t *out, unsigned &arrive)
{
    const int lane = threadIdx.x & 63;
    const int steps = len + 2 * VIT_EXTRA, npairs = k9_pairs(len);
    unsigned long long *stage = (unsigned long long *)&sm.metric[0][0];
    const uint8_t *db8 = (const uint8_t *)stage;
    for (int c = c_hi - 1; c >= c_lo; c--) {
        if (c == c_out - 1) arrive = state;
        const int p0 = c << 5, np = min(32, npairs - p0);
        for (int k = lane; k < 8 * np; k += 64) stage[k] = dec[(size_t)p0 * 8 + k];
        WAVE_LDS_SYNC();
        unsigned long long obits = 0;                           // output bits of steps 2 p0 .. 2 p0 + 63
        for (int s = np - 1; s >= 0; s--) {
            const unsigned i1 = state >> 7, i0 = (state >> 6) & 1u, L = state & 63u;
            const unsigned q = db8[64 * s + L];                  // lane L's decision byte of this step pair: one broadcast read
            const unsigned xh = (q >> (4 + 2 * i1 + i0)) & 1u;
            const unsigned xl = (q >> (2 * i0 + xh)) & 1u;
            obits = (obits << 2) | (unsigned long long)(i0 | (i1 << 1));    // the pair walked last (s = 0) ends in bits 0..1
            state = (unsigned)wave_uniform((int)((L << 2) | (xh << 1) | xl));
        }
        WAVE_LDS_SYNC();
        if (lane == 0 && c < c_out) {
            const int wl = 2 * c - 1, wh = 2 * c;
            if (wl >= 0 && wl * 32 < len) out[wl] = (uint32_t)obits;
            if (wh * 32 < len && 2 * p0 + 32 < steps) out[wh] = (uint32_t)(obits >> 32);
        }
    }
    return state;
}

__device__ inline void viterbi_k9_wave(const int8_t *coded, int len, unsigned g0, unsigned g1, unsigned g2,
                                       unsigned long long *dec, uint32_t *out, K9WSmem &sm, int phases = 3)
{
    const int lane = threadIdx.x & 63;
    const K9Signs sg = k9_signs(lane, g0, g1, g2);
    const int npairs = k9_pairs(len), nchunks = k9_chunks(len);
    for (int k = 0; k < 4; k++) sm.metric[0][4 * lane + k] = 0;   // reset_decoder: all-zero for tail biting
    WAVE_LDS_SYNC();
    const int cur = (phases & 1) ? k9_forward_chunks(coded, len, sg, dec, sm, 0, nchunks, 0, nullptr) : 0;
    unsigned state = k9_end_state(*(const int4 *)&sm.metric[cur][4 * lane]);
    __threadfence_block();
    __syncthreads();
    unsigned arrive = 0;
    if (phases & 2) k9_traceback_chunks(dec, len, sm, state, (npairs + 31) >> 5, 0, (npairs + 31) >> 5, out, arrive);
    __threadfence_block();
    __syncthreads();
}

// ---- the same decode in segment waves ---------------------------------------------------------------------------------
// FORWARD.  The chunks of a frame are cut into up to K9_GMAX segments, one wave each, all running at once.  Segment g > 0 cannot
// know the metrics its first step starts from, so it starts `warm` chunks early from all-zero metrics -- survivor paths merge
// within a few constraint lengths, after which metric DIFFERENCES no longer depend on where the wave started -- and notes the
// metrics it reaches its first own step with (snap).  Decisions depend on metric differences only (int32 sums, no saturation,
// no normalisation): k9_forward_fix walks the boundaries in order and accepts segment g iff snap[g] - snap[g][0] equals the TRUE
// end metrics of segment g - 1 minus their element 0; otherwise it re-runs segment g from those.  Exact for any segment count and
// any warm-up, including 0 (the test hook that forces every repair).
// TRACEBACK.  Segment g < last starts K9_TB_RUNIN chunks above its own chunks from state 0 -- survivors merge going backwards
// too -- and notes the state it enters its own chunks with (arrive) and leaves them with (leave); the last segment starts from
// the true end state.  k9_traceback_fix walks down from the last segment: segment g is accepted iff arrive[g] is the state the
// segment above truly left with, else it is walked again from that state.  Output words are per chunk, so a repair rewrites
// exactly the words of its segment.
// K9_GMAX, K9_WARM (chunks of 64 step pairs) and K9_TB_RUNIN (chunks of 32 step pairs): nrsc5_dev.h

__host__ __device__ inline int k9_seg_chunks(int len, int G) { return (k9_chunks(len) + G - 1) / G; }
__host__ __device__ inline int k9_seg_count(int len, int G) { const int per = k9_seg_chunks(len, G); return (k9_chunks(len) + per - 1) / per; }

__device__ inline void k9_forward_segment(const int8_t *coded, int len, unsigned g0, unsigned g1, unsigned g2, unsigned long long *dec,
                                          K9Meta &meta, K9WSmem &sm, int g, int G, int warm)
{
    const int lane = threadIdx.x & 63;
    const int nch = k9_chunks(len), per = k9_seg_chunks(len, G);
    const int c0 = g * per, c1 = min(nch, c0 + per);
    if (c0 >= nch) return;                                     // wave-uniform
    const K9Signs sg = k9_signs(lane, g0, g1, g2);
    for (int k = 0; k < 4; k++) sm.metric[0][4 * lane + k] = 0;
    WAVE_LDS_SYNC();
    const int cur = k9_forward_chunks(coded, len, sg, dec, sm, g ? max(0, c0 - warm) : 0, c1, c0, g ? meta.snap[g] : nullptr);
    *(int4 *)&meta.uend[g][4 * lane] = *(const int4 *)&sm.metric[cur][4 * lane];
}

// one wave per frame, after every segment wave has finished: returns the end state of the frame
__device__ inline unsigned k9_forward_fix(const int8_t *coded, int len, unsigned g0, unsigned g1, unsigned g2, unsigned long long *dec,
                                          K9Meta &meta, K9WSmem &sm, int G, unsigned *stats)
{
    const int lane = threadIdx.x & 63;
    const int nch = k9_chunks(len), per = k9_seg_chunks(len, G), nseg = k9_seg_count(len, G);
    const K9Signs sg = k9_signs(lane, g0, g1, g2);
    int4 tend = *(const int4 *)&meta.uend[0][4 * lane];        // true end metrics of the segment below, up to a constant
    unsigned repairs = 0;
    for (int g = 1; g < nseg; g++) {
        const int4 a = *(const int4 *)&meta.snap[g][4 * lane];
        const int a0 = wave_readlane(a.x, 0), b0 = wave_readlane(tend.x, 0);
        const bool same = a.x - a0 == tend.x - b0 && a.y - a0 == tend.y - b0 && a.z - a0 == tend.z - b0 && a.w - a0 == tend.w - b0;
        if (__all(same)) { tend = *(const int4 *)&meta.uend[g][4 * lane]; continue; }
        *(int4 *)&sm.metric[0][4 * lane] = tend;
        WAVE_LDS_SYNC();
        const int c0 = g * per, c1 = min(nch, c0 + per);
        const int cur = k9_forward_chunks(coded, len, sg, dec, sm, c0, c1, c0, nullptr);
        tend = *(const int4 *)&sm.metric[cur][4 * lane];
        WAVE_LDS_SYNC();
        repairs++;
    }
    if (stats && lane == 0) { atomicAdd(&stats[0], (unsigned)(nseg - 1)); if (repairs) atomicAdd(&stats[1], repairs); }
    return k9_end_state(tend);
}

__device__ inline void k9_traceback_segment(const unsigned long long *dec, int len, K9Meta &meta, K9WSmem &sm, uint32_t *out, int g, int G, int runin)
{
    const int nch = k9_chunks(len), per = k9_seg_chunks(len, G), nseg = k9_seg_count(len, G);
    if (g >= nseg) return;                                     // wave-uniform
    const int ntb = (k9_pairs(len) + 31) >> 5;
    const int lo = 2 * g * per, hi = min(ntb, 2 * min(nch, (g + 1) * per));
    const bool last = g == nseg - 1;
    unsigned arrive = last ? meta.end_state : 0u;
    const unsigned leave = k9_traceback_chunks(dec, len, sm, arrive, last ? hi : min(ntb, hi + runin), lo, hi, out, arrive);
    if ((threadIdx.x & 63) == 0) { meta.arrive[g] = arrive; meta.leave[g] = leave; }
}

// one wave per frame, after every traceback segment wave has finished
__device__ inline void k9_traceback_fix(const unsigned long long *dec, int len, K9Meta &meta, K9WSmem &sm, uint32_t *out, int G, unsigned *stats)
{
    const int nch = k9_chunks(len), per = k9_seg_chunks(len, G), nseg = k9_seg_count(len, G);
    const int ntb = (k9_pairs(len) + 31) >> 5;
    unsigned truth = (unsigned)wave_uniform((int)meta.leave[nseg - 1]), repairs = 0;
    for (int g = nseg - 2; g >= 0; g--) {
        if ((unsigned)wave_uniform((int)meta.arrive[g]) == truth) { truth = (unsigned)wave_uniform((int)meta.leave[g]); continue; }
        const int lo = 2 * g * per, hi = min(ntb, 2 * min(nch, (g + 1) * per));
        unsigned arrive = 0;
        truth = k9_traceback_chunks(dec, len, sm, truth, hi, lo, hi, out, arrive);
        repairs++;
    }
    if (stats && (threadIdx.x & 63) == 0) { atomicAdd(&stats[2], (unsigned)(nseg - 1)); if (repairs) atomicAdd(&stats[3], repairs); }
    __threadfence_block();
    __syncthreads();
}

// re-encode the decoded (still scrambled) bits and count sign disagreements at unpunctured positions
// (bit_errors, decode.c:234-261); returns the block-wide total in every work-item
__device__ inline int am_bit_errors(const int8_t *coded, const uint32_t *bits, int len, unsigned g0, unsigned g1, unsigned g2,
                                    unsigned pmask, int plen, int *red /* [4] */)
{
    int errors = 0;
    // puncture phase of coded bit 3 i: the period belongs to the frame's code, so it is carried along the loop, not divided by
    int ph = (3 * (int)threadIdx.x) % plen;
    const int dph = (3 * (int)blockDim.x) % plen;
    for (int i = threadIdx.x; i < len; i += blockDim.x) {
        unsigned r = 0;                                        // r bit 8-k = bits[i-k]
#pragma unroll
        for (int k = 0; k < 9; k++) {
            int q = i - k; if (q < 0) q += len;
            r |= ((bits[q >> 5] >> (q & 31)) & 1u) << (8 - k);
        }
        const int j = 3 * i;
        const int ph1 = ph + 1 < plen ? ph + 1 : ph + 1 - plen, ph2 = ph + 2 < plen ? ph + 2 : ph + 2 - plen;
        if (((pmask >> ph) & 1u) && ((coded[j] > 0) != (int)(__popc(r & g0) & 1))) errors++;
        if (((pmask >> ph1) & 1u) && ((coded[j + 1] > 0) != (int)(__popc(r & g1) & 1))) errors++;
        if (((pmask >> ph2) & 1u) && ((coded[j + 2] > 0) != (int)(__popc(r & g2) & 1))) errors++;
        ph += dph; if (ph >= plen) ph -= plen;
    }
    errors = wave_sum_i32(errors);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = errors;
    __syncthreads();
    int total = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) total += red[w];
    return total;
}

constexpr unsigned GEN_E1_0 = 0561, GEN_E1_1 = 0657, GEN_E1_2 = 0711;     // decode.c:47-53
constexpr unsigned GEN_E2_0 = 0561, GEN_E2_1 = 0753, GEN_E2_2 = 0711;     // decode.c:55-61
constexpr unsigned PUNCT_E1 = 0x7f6d, PUNCT_E2 = 0x0d;                    // bit k = pattern[k]: {1,0,1,1,0,1,1,0,1,1,1,1,1,1,1}, {1,0,1,1,0,0}

}  // namespace nrsc5
