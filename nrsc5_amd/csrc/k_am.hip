// AM (hybrid MA1 / all-digital MA3) path for gfx950.  Replaces, for NRSC5_MODE_AM:
//   decimate_samples' 5-stage 32:1 cascade (input.c:70-91)                         -> k_am_decimate_cu8 (k_am_decimate.hip)
//   acquire_process incl. the AM carrier regression (acquire.c:98-263)             -> k_am_block (fused)
//   sync_push / sync_process_am, find_ref_am, find_block_am (sync.c:209-252,612-767)-> k_am_block
//   decode_process_pids_am (decode.c:474-505)                                      -> k_am_block tail
//   decode_process_p1_p3_am, nrsc5_conv_decode_e1 / _e2_e3 (decode.c:507-554)      -> k_am_viterbi, k_am_decode_* (k_am_decode.hip; the
//                                                                                     trellis itself: viterbi_k9.h)
//   interleaver_ma1 incl. the 3-frame diversity delay (decode.c:74-231)            -> k_am_interleave
// This file holds the block step and the interleaver.
//
// The AM stream is 32 x slower than FM (46.5 kS/s), so one workgroup owns one stream for a whole block:
// the 32 x 256-point FFTs, the carrier line fit and sync_process_am all run out of one 64 KB LDS tile and
// only hard symbols (3.2 KB per block) go back to HBM.  The K=9 trellis has 256 states = one per work-item.
#include <atomic>
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "fastmath.h"
#include "wave_ops.h"
#include "l2_header.h"
#include "viterbi_k9.h"

namespace nrsc5 {

// =====================================================================================================
// the block step
// =====================================================================================================
struct AmBlockSmem {
    float2 X[NSYM * AM_FFT];        // 64 KB: coarse-acquisition scratch, then the 32 symbol spectra (natural order)
    float2 tw[AM_FFT / 2];
    float shape[AM_SYM];
    float2 mult[4][AM_PW];
    float marg[2][AM_PW];
    float2 carrier[NSYM];
    float magsum[2 * 53 + 1];
    float red_mag[16]; int red_idx[16]; float2 red_v[16];
    uint8_t pids_sym[2 * NSYM];
    int8_t pids_coded[3 * PIDS_LEN];
    uint32_t pids_out[3];
    // block-uniform scalars produced by work-item 0
    int active, fine, samperr, ma3, refmask;
    int deliver;                // replay: P1 PDU this block delivered (0..7), -1: none
    double theta, dtheta;
    float2 step270, step256;        // e^{i 270 dtheta}, e^{i 256 dtheta}
    float dphi[NSYM];           // carrier phase advance per symbol (line fit), one work-item each
    double targ;                // argument handed from work-item 0 to the work-items that evaluate its cosine / sine
    int bc_now, psmi_now, rdbi_now;   // the stream's block count / service mode / RDBI after the reference decode (block-uniform copies)
};
// the PIDS trellis runs after the spectra are consumed: its scratch aliases the head of X
static_assert(sizeof(K9Smem) + 4 * (PIDS_LEN + 64) * sizeof(unsigned long long) <= sizeof(float2) * NSYM * AM_FFT, "PIDS scratch must fit in X");

__device__ inline float2 cmulf(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline float2 cdivf(float2 a, float2 b)
{
    const float d = b.x * b.x + b.y * b.y;
    return make_float2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}
__device__ inline unsigned bitrev8(unsigned v) { return __brev(v) >> 24; }

// sync.c:37-88
__device__ inline unsigned slice4(float f) { return f < -1 ? 0u : f < 0 ? 2u : f < 1 ? 3u : 1u; }
__device__ inline unsigned slice8(float f) { return f < -3 ? 0u : f < -2 ? 4u : f < -1 ? 6u : f < 0 ? 2u : f < 1 ? 3u : f < 2 ? 7u : f < 3 ? 5u : 1u; }
__device__ inline unsigned sym_qpsk(float2 c) { return (c.x < 0 ? 0u : 1u) | (c.y < 0 ? 0u : 2u); }
__device__ inline unsigned sym_qam16(float2 c) { return slice4(c.x) | (slice4(c.y) << 2); }
__device__ inline unsigned sym_qam64(float2 c) { return slice8(c.x) | (slice8(c.y) << 3); }

__device__ inline float half_turn_diff(float a, float b)   // phase_diff, sync.c:284-290
{
    float d = a - b;
    while (d > (float)(M_PI / 2)) d = (float)((double)d - M_PI);
    while (d < (float)(-M_PI / 2)) d = (float)((double)d + M_PI);
    return d;
}

// Mix one block down with the NCO (phase theta + dtheta * sample), fold the cyclic prefix (rotated by 121 samples:
// carrier phases are referenced to the symbol centre, acquire.c:239-247) and leave the 32 inputs in NATURAL order for the
// 16 x 16 transform below.  Work-item j owns input slot j of every symbol.
template <int NT> __device__ inline void am_fold(AmBlockSmem &sm, const c16 *win, int samperr, double theta, float2 step270, float2 step256)
{
    // work-item (j, g): sample j of the eight symbols of group g; the phasor is evaluated in closed form at the head of every
    // group and advanced by recurrence inside it, whatever the block size (256 work-items take the four groups in turn, 512
    // two each), so that both launch shapes produce the same bits
    const int j = threadIdx.x & 255;
    const unsigned slot = (unsigned)(j + (AM_FFT - AM_CP) / 2) & 255u;
    constexpr int NG = (NSYM / 8) / (NT >> 8);
    // every sample this work-item will mix, requested before the first is used: one at a time behind the phasor recurrence the 16 loads of a
    // work-item were 16 dependent trips to L2 / HBM (the first fold of a block: 33 k of its 139 k shader cycles; profiles/r05_am_phases.txt)
    c16 a[NG][8], c[NG][8];
#pragma unroll
    for (int q = 0; q < NG; q++) {
        const int g = ((int)threadIdx.x >> 8) + q * (NT >> 8);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            a[q][k] = win[(8 * g + k) * AM_SYM + j + samperr];
            c[q][k] = win[(8 * g + k) * AM_SYM + (j < AM_CP ? j + AM_FFT : j) + samperr];      // (work-items >= AM_CP: the same line again, unused)
        }
    }
#pragma unroll
    for (int q = 0; q < NG; q++) {
        const int g = ((int)threadIdx.x >> 8) + q * (NT >> 8);
        float2 p;
        {
            double th = theta + sm.dtheta * (double)(j + g * 8 * AM_SYM);
            th -= 2 * M_PI * rint(th / (2 * M_PI));
            float sn, cs; sincosf((float)th, &sn, &cs);
            p = make_float2(cs, sn);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int i = 8 * g + k;
            float2 v = cmulf(p, make_float2((float)a[q][k].r / 32767.0f, (float)a[q][k].i / 32767.0f));    // cq15_to_cf, defines.h:106
            if (j < AM_CP) {
                const float2 w = cmulf(cmulf(p, step256), make_float2((float)c[q][k].r / 32767.0f, (float)c[q][k].i / 32767.0f));
                const float sa = sm.shape[j], sb = sm.shape[j + AM_FFT];
                v = make_float2(sa * v.x + sb * w.x, sa * v.y + sb * w.y);
            }
            sm.X[i * AM_FFT + slot] = v;
            p = cmulf(p, step270);
        }
    }
}

// forward 4-point DFT in place, natural order
__device__ __forceinline__ void am_dft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3)
{
    const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y), d = make_float2(a1.x - a3.x, a1.y - a3.y);
    const float2 t3 = make_float2(d.y, -d.x);                  // (a1 - a3) * (-j)
    a0 = make_float2(t0.x + t2.x, t0.y + t2.y); a1 = make_float2(t1.x + t3.x, t1.y + t3.y);
    a2 = make_float2(t0.x - t2.x, t0.y - t2.y); a3 = make_float2(t1.x - t3.x, t1.y - t3.y);
}
// forward 16-point DFT in place: input v[n], output X[4 k1 + k2] in v[4 k2 + k1]
__device__ __forceinline__ void am_dft16(float2 *v)
{
#pragma unroll
    for (int n1 = 0; n1 < 4; n1++) am_dft4(v[n1], v[n1 + 4], v[n1 + 8], v[n1 + 12]);     // v[n1 + 4 k2] = Y[n1][k2]
    const float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, c2 = 0.70710678118654752440f;
    // W16^(n1 k2) = e^{-2 pi i n1 k2 / 16}
    v[5] = cmulf(v[5], make_float2(c1, -s1));     // 1
    v[6] = cmulf(v[6], make_float2(c2, -c2));     // 2
    v[7] = cmulf(v[7], make_float2(s1, -c1));     // 3
    v[9] = cmulf(v[9], make_float2(c2, -c2));     // 2
    v[10] = make_float2(v[10].y, -v[10].x);       // 4: -j
    v[11] = cmulf(v[11], make_float2(-c2, -c2));  // 6
    v[13] = cmulf(v[13], make_float2(s1, -c1));   // 3
    v[14] = cmulf(v[14], make_float2(-c2, -c2));  // 6
    v[15] = cmulf(v[15], make_float2(-c1, s1));   // 9
#pragma unroll
    for (int k2 = 0; k2 < 4; k2++) am_dft4(v[4 * k2], v[4 * k2 + 1], v[4 * k2 + 2], v[4 * k2 + 3]);
}

// 32 x 256-point forward FFT in LDS, natural order in and out: 256 = 16 x 16, sixteen points per work-item in registers, ONE exchange through the tile
// (n = 16 a + b, k = c + 16 d: work-item (symbol, b) transforms over a and applies W256^(b c); work-item (symbol, c) transforms over b).  The
// exchange is in place: Y[c][b] sits at c * 16 + (b ^ c), which keeps both the writes (b runs across the work-items) and the reads (c runs across
// them: a plain row-major tile would put all sixteen on one bank) conflict-free without a second buffer.  Round 4's form -- eight radix-2 passes, each
// a read-modify-write of the whole 64 KB tile behind a barrier -- was 21 k of the block's 139 k shader cycles.
template <int NT> __device__ inline void am_fft_all(AmBlockSmem &sm)
{
    static_assert((NSYM * 16) % NT == 0, "whole rounds");
    for (int id0 = 0; id0 < NSYM * 16; id0 += NT) {
        const int id = id0 + (int)threadIdx.x, n = id >> 4, l = id & 15;
        float2 *x = sm.X + n * AM_FFT;
        float2 v[16];
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 16; a++) v[a] = x[16 * a + l];                        // b = l
        am_dft16(v);
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < 4; k2++)
#pragma unroll
            for (int k1 = 0; k1 < 4; k1++) {
                const int c = 4 * k1 + k2, m = l * c;                             // W256^(b c), b c <= 225
                float2 w = sm.tw[m & 127];
                if (m & 128) w = make_float2(-w.x, -w.y);
                x[c * 16 + (l ^ c)] = c ? cmulf(v[4 * k2 + k1], w) : v[4 * k2 + k1];
            }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 16; b++) v[b] = x[l * 16 + (b ^ l)];                  // c = l
        am_dft16(v);
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < 4; k2++)
#pragma unroll
            for (int k1 = 0; k1 < 4; k1++) x[l + 16 * (4 * k1 + k2)] = v[4 * k2 + k1];
    }
    __syncthreads();
}

// spectrum bin `off` relative to the carrier (fftshift folded into the index), symbol n
__device__ inline float2 &am_bin(AmBlockSmem &sm, int off, int n) { return sm.X[n * AM_FFT + (off & 255)]; }

// e^{i 270 dtheta}, e^{i 256 dtheta} from sm.dtheta: four double-precision cosines / sines, one per wave (work-items 0, 64, 128, 192), instead of four in
// a row on work-item 0.  Same functions of the same arguments: the same bits.  Callers put a barrier before (sm.dtheta) and after.
__device__ __forceinline__ void am_nco_steps(AmBlockSmem &sm)
{
    const int tid = threadIdx.x;
    if ((tid & 63) == 0 && tid < 256) {
        const int w = tid >> 6;
        const double x = sm.dtheta * (double)(w < 2 ? AM_SYM : AM_FFT);
        float v;
        if (fabs(x) <= 0.25) { double c, sn; small_cos_sin(x, c, sn); v = (w & 1) ? (float)sn : (float)c; }   // integer CFO 0 (every block once tuned): the series of fastmath.h, a few ulps of a double
        else v = (w & 1) ? (float)sin(x) : (float)cos(x);
        float2 &dst = w < 2 ? sm.step270 : sm.step256;
        if (w & 1) dst.y = v; else dst.x = v;
    }
}

// 256 work-items per stream (the in-order K=9 PIDS trellis below owns one state per work-item).  Every wide phase strides by the
// block size, but 1024 work-items were measured SLOWER in the window pipeline (am-cs16 88.6 -> 108.4 ms): a 16-wave workgroup with
// 64 KB of LDS waits for a whole CU's worth of slots while the decode streams keep the chip full of long one-wave trellis passes.
// (NT, the block size, is a template constant: read as blockDim.x it is two dependent global loads -- implicit-argument pointer, dispatch packet -- in
// front of the first loop that strides by it; profiles/r04_mixfft_phases.txt)
// DUMP (nrsc5hip_stage_am_block, tests/am_checks.py): the stage hook's instantiations take two more arguments, float2 *x [NSYM * AM_FFT] and float2 *mult [4 * AM_PW], and
// copy the tile behind the sideband combine and the equaliser taps out to them.  The production instantiations (DUMP = false, an empty pack) are the code they were.
template <int NT, bool DUMP = false, typename... Dump>
__global__ __launch_bounds__(NT) void k_am_block(DevTables tb, DevBuffers db, const int *ids, int pipeline, int parity, int slot, Dump... dump)
{
    wave_set_priority_high();                                  // block-step chain = critical path; the decode waves run at priority 0
    const int s = stream_of(ids, blockIdx.x);
    StreamState &st = db.state[s];
    AmStream &am = db.am[s];
    HIP_DYNAMIC_SHARED(uint8_t, smem_raw)
    AmBlockSmem &sm = *(AmBlockSmem *)smem_raw;
    const int tid = threadIdx.x;
    static_assert(NT >= 256 && NT % 256 == 0, "four waves share the NCO's cosines / sines; the fold strides by groups of 256");
    const bool ready = st.wr - st.rd >= AM_WIN;                 // block-uniform
    if (tid == 0) {
        am.dec_bc = -1; st.active = ready ? 1 : 0;
        sm.deliver = -1;
    }
    __syncthreads();
    if (!ready) return;
    const c16 *win = db.q15 + (size_t)s * db.q15_cap + (st.rd - st.base);
    const int state_before = st.sync_state;
    // phase instrumentation (nrsc5hip_debug_tune NRSC5HIP_TUNE_SYNC_PHASES; tools/gpu_am_phases.py): shader cycles of stream 0's workgroup between the marks
    __shared__ long long am_tstamp;
    if (db.sync_phase_cycles && s == 0 && tid == 0) am_tstamp = (long long)clock64();
#define AM_MARK(i) do { if (db.sync_phase_cycles && s == 0 && tid == 0) { const long long now = (long long)clock64(); db.sync_phase_cycles[i] += now - am_tstamp; am_tstamp = now; } } while (0)

    for (int k = tid; k < AM_FFT / 2; k += NT) sm.tw[k] = tb.am_twiddle[k];
    for (int k = tid; k < AM_SYM; k += NT) sm.shape[k] = tb.am_shape[k];

    // ---- coarse acquisition while not FINE (acquire.c:120-158 with the AM filter / geometry) ------------------
    if (state_before != SYNC_FINE) {
        c16 *filt = (c16 *)sm.X;                               // [AM_WIN]
        float2 *sums = (float2 *)(filt + AM_WIN + 2);          // [AM_SYM], 8-byte aligned (AM_WIN even)
        for (int t = tid; t < AM_WIN; t += NT) {
            int sr = 0, si = 0;
#pragma unroll
            for (int i = 1; i < 16; i++) {
                const int ka = t - 31 + i, kb = t - 31 + (32 - i);
                const c16 xa = ka >= 0 ? win[ka] : st.fir_hist[31 + ka];
                const c16 xb = kb >= 0 ? win[kb] : st.fir_hist[31 + kb];
                const int q = tb.am_acq_q15[i];
                sr = (int16_t)(sr + (((xa.r + xb.r) * q) >> 15));
                si = (int16_t)(si + (((xa.i + xb.i) * q) >> 15));
            }
            const int kc = t - 15;
            const c16 xc = kc >= 0 ? win[kc] : st.fir_hist[31 + kc];
            const int q = tb.am_acq_q15[16];
            sr = (int16_t)(sr + ((xc.r * q) >> 15));
            si = (int16_t)(si + ((xc.i * q) >> 15));
            c16 y; y.r = (int16_t)sr; y.i = (int16_t)si;
            filt[t] = y;
        }
        __syncthreads();
        for (int i = tid; i < AM_SYM; i += NT) {
            float sr = 0.0f, si = 0.0f;
            for (int j = 0; j < NSYM; j++) {
                const c16 qa = filt[i + j * AM_SYM], qb = filt[i + j * AM_SYM + AM_FFT];
                const float ax = (float)qa.r / 32767.0f, ay = (float)qa.i / 32767.0f;
                const float bx = (float)qb.r / 32767.0f, by = -((float)qb.i / 32767.0f);      // conjf
                sr += ax * bx - ay * by; si += ax * by + ay * bx;
            }
            sums[i] = make_float2(sr, si);
        }
        __syncthreads();
        float best_mag = -1.0f; int best_i = 0x7fffffff; float2 best_v = make_float2(0.0f, 0.0f);
        for (int i = tid; i < AM_SYM; i += NT) {
            float vr = 0.0f, vi = 0.0f;
            int k = i;
            for (int j = 0; j < AM_CP; j++) {
                const float2 z = sums[k];
                vr += (z.x * sm.shape[j]) * sm.shape[j + AM_FFT];
                vi += (z.y * sm.shape[j]) * sm.shape[j + AM_FFT];
                if (++k == AM_SYM) k = 0;
            }
            const float mag = vr * vr + vi * vi;
            if (mag > best_mag) { best_mag = mag; best_i = i; best_v = make_float2(vr, vi); }
        }
        for (int m = 32; m >= 1; m >>= 1) {                    // first maximum in index order wins
            const float om = __shfl_xor(best_mag, m); const int oi = __shfl_xor(best_i, m);
            const float ox = __shfl_xor(best_v.x, m), oy = __shfl_xor(best_v.y, m);
            if (om > best_mag || (om == best_mag && oi < best_i)) { best_mag = om; best_i = oi; best_v = make_float2(ox, oy); }
        }
        if ((tid & 63) == 0) { sm.red_mag[tid >> 6] = best_mag; sm.red_idx[tid >> 6] = best_i; sm.red_v[tid >> 6] = best_v; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NT / 64; w++)
                if (sm.red_mag[w] > best_mag || (sm.red_mag[w] == best_mag && sm.red_idx[w] < best_i)) { best_mag = sm.red_mag[w]; best_i = sm.red_idx[w]; best_v = sm.red_v[w]; }
            st.coarse_samperr = (best_i + AM_SYM - 15) % AM_SYM;       // FILTER_DELAY, acquire.c:149
            st.coarse_re = best_v.x; st.coarse_im = best_v.y;
        }
        if (tid < 31) {
            st.fir_hist[tid] = win[AM_WIN - 31 + tid];
            const long long p = stale_start(st.stale.fir_pushed[MODE_AM], AM_WIN, 31);     // filter_am's compaction inside this block (>= 0: AM_WIN > 2 * 2017)
            if (p != STALE_NONE) st.stale.fir[MODE_AM][tid] = win[p + tid];
        }
        __syncthreads();
        if (tid == 0) st.stale.fir_pushed[MODE_AM] += AM_WIN;
    }

    AM_MARK(0);                                                // tables + coarse acquisition (while not FINE)
    // ---- per-block bookkeeping (top of acquire_process, acquire.c:110-119,153-168) -------------------------------
    BlockRecord &rec = db.records[(size_t)s * db.rec_cap + (st.nblocks % db.rec_cap)];
    if (tid == 0) {
        atomicAdd(&db.counters[0], 1);
        BlockRecord r;
        r.flags = REC_PROCESSED; r.state_before = state_before; r.state_after = 0;
        r.samperr = 0; r.cfo = 0; r.keep = 0; r.bc = 0; r.psmi = 0; r.cfo_wait = 0; r.next_samperr = 0;
        r.prev_angle = 0; r.phase_re = 0; r.phase_im = 0; r.next_angle = 0; r.freq_offset = 0; r.mer_lb = 0; r.mer_ub = 0;
        r.ber = 0; r.p1_slot = -1; r.bc_decoded = -1; r.pids[0] = r.pids[1] = r.pids[2] = 0; r.sis = 0;
        // the state words this section reads, in one burst (each behind the branch that needs it they were a chain of L2 round trips)
        const int st_samperr = st.samperr, st_cfo = st.cfo, st_psmi = st.psmi, st_coarse_samperr = st.coarse_samperr;
        int sync_state = st.sync_state;
        const float st_prev_angle = st.prev_angle, st_coarse_re = st.coarse_re, st_coarse_im = st.coarse_im;
        const double st_theta = st.theta;
        int samperr; float angle;
        if (state_before == SYNC_FINE) {
            samperr = AM_SYM / 2 + st_samperr; st.samperr = 0;
            // sync_t.angle is only written by the FM path: zero, except in the first synchronised block after a reset that followed an FM session (nrsc5hip_stream_reset
            // keeps it as sync_reset does) -- acquire.c:115-118 consumes it whatever the mode
            angle = st_prev_angle + -st.angle;
            st.angle = 0.0f; st.prev_angle = angle;
        } else {
            samperr = st_coarse_samperr;
            float sn, cs; ref_sincosf(-st_prev_angle, sn, cs);   // cexpf(I * -prev_angle), acquire.c:153: glibc's sincosf restated (fastmath.h)
            const float pr = st_coarse_re * cs - st_coarse_im * sn;
            const float pi = st_coarse_re * sn + st_coarse_im * cs;
            const float angle_diff = ref_atan2f(pi, pr);
            const float angle_factor = (st_prev_angle != 0.0f) ? 0.25f : 1.0f;
            angle = st_prev_angle + (angle_diff * angle_factor);
            st.prev_angle = angle;
            if (sync_state != SYNC_COARSE) { r.flags |= REC_TO_COARSE; sync_state = SYNC_COARSE; st.sync_state = SYNC_COARSE; }
        }
        rec = r;
        angle = (float)((double)angle - 2 * M_PI * st_cfo);    // acquire.c:164
        const float dth = angle / AM_FFT;
        double th = st_theta + (double)(-(float)(AM_SYM / 2 - samperr) * angle / AM_FFT);  // acquire.c:166
        th -= 2 * M_PI * rint(th / (2 * M_PI));
        sm.theta = th; sm.targ = (double)dth;
        sm.samperr = samperr; sm.fine = sync_state == SYNC_FINE; sm.ma3 = st_psmi == AM_MA3;
    }
    __syncthreads();
    // phase_increment = cexpf(angle / fft * I) (acquire.c:168; kept for the slope correction below): glibc's sincosf of the float argument, restated bit for bit
    // (ref_sincosf, fastmath.h) -- round 6; until round 5 a double-precision cosine and sine on two waves, rounded once (another float for 1.3 % of arguments) and
    // two barriers and ~8 k cycles more.  The effective step of the closed-form oscillator is the angle of that rounded pair.
    if (tid == 0) {
        float sn, cs; ref_sincosf((float)sm.targ, sn, cs);       // (sm.targ holds the float dth exactly)
        sm.red_v[0] = make_float2(cs, sn);
        const double t = (double)sn / (double)cs;
        sm.dtheta = (cs > 0.0f && fabs(t) <= 0.26) ? small_atan(t) : atan2((double)sn, (double)cs);
    }
    __syncthreads();
    am_nco_steps(sm);
    __syncthreads();
    const int samperr = sm.samperr;
    const bool fine_at_top = sm.fine != 0;
    AM_MARK(1);                                                // bookkeeping + NCO set-up (one work-item, double-precision trigonometry)

    // ---- pass 1: phase of the analog carrier per symbol, line fit over the block (acquire.c:170-235) -------------
    am_fold<NT>(sm, win, samperr, sm.theta, sm.step270, sm.step256);
    AM_MARK(2);                                                // pass-1 fold
    if (fine_at_top) {
        // only the carrier bin is needed: sum of the folded inputs (bin 0 before fftshift)
        __syncthreads();
        if (tid < 256) {
            const int n = tid >> 3, part = tid & 7;            // 8 work-items per symbol, 32 inputs each
            float sr = 0.0f, si = 0.0f;
            for (int k = 0; k < 32; k++) { const float2 v = sm.X[n * AM_FFT + part * 32 + k]; sr += v.x; si += v.y; }
            for (int m = 4; m >= 1; m >>= 1) { sr += __shfl_xor(sr, m); si += __shfl_xor(si, m); }
            if (part == 0) sm.carrier[n] = make_float2(sr, si);
        }
    } else {
        am_fft_all<NT>(sm);
        if (tid < NSYM) sm.carrier[tid] = am_bin(sm, 0, tid);
        if (tid <= 2 * 53) {                                   // |bins| summed over the block, carrier +-53
            float acc = 0.0f;
            for (int n = 0; n < NSYM; n++) { const float2 v = am_bin(sm, tid - 53, n); acc += sqrtf(v.x * v.x + v.y * v.y); }
            sm.magsum[tid] = acc;
        }
    }
    __syncthreads();
    // The line fit (acquire.c:199-231).  The phase advance of every symbol -- a complex division and an arc tangent, 32 of them in a row on one
    // work-item as the reference's loop is written -- is a function of two neighbouring carriers only: one work-item each; the running sums stay
    // one sequential chain in the reference's order (same additions, same bits).
    if (tid < NSYM) {
        const float2 c = sm.carrier[tid];
        float d;
        if (tid == 0) d = ref_atan2f(c.y, c.x);
        else { const float2 q = cdivf(c, sm.carrier[tid - 1]); d = ref_atan2f(q.y, q.x); }
        sm.dphi[tid] = d;
    }
    __syncthreads();
    if (tid == 0) {
        float y = 0, sum_y = 0, sum_xy = 0, sum_x2 = 0;
        for (int i = 0; i < NSYM; i++) {
            const float x = AM_SYM * (i - (float)(NSYM - 1) / 2);
            if (i == 0) y = sm.dphi[0];
            else y += sm.dphi[i];
            sum_y += y; sum_xy += x * y; sum_x2 += x * x;
        }
        if (!fine_at_top) {
            float max_mag = -1.0f; int max_index = -1;
            for (int j = 0; j <= 2 * 53; j++) if (sm.magsum[j] > max_mag) { max_mag = sm.magsum[j]; max_index = j; }
            st.cfo += max_index - 53;                          // acquire_cfo_adjust: effective from the next block
        }
        const float slope = sum_xy / sum_x2;
        const float a = -sum_y / NSYM + slope * NSYM * AM_SYM / 2;
        const float corr = (float)((double)a - 0.06);          // acquire.c:233-234
        double th = sm.theta + (double)corr;
        th -= 2 * M_PI * rint(th / (2 * M_PI));
        sm.theta = th; sm.targ = (double)slope;
    }
    __syncthreads();
    // phase_increment *= cexpf(-slope I) (acquire.c:232): glibc's sincosf of -slope (ref_sincosf), then the float complex product of the two rounded unit vectors
    if (tid == 0) {
        float rs, rc; ref_sincosf(-(float)sm.targ, rs, rc);     // (sm.targ holds the float slope exactly)
        const float2 inc = sm.red_v[0];
        const float2 inc2 = make_float2(inc.x * rc - inc.y * rs, inc.x * rs + inc.y * rc);
        const double t = (double)inc2.y / (double)inc2.x;
        sm.dtheta = (inc2.x > 0.0f && fabs(t) <= 0.26) ? small_atan(t) : atan2((double)inc2.y, (double)inc2.x);
    }
    __syncthreads();
    am_nco_steps(sm);
    __syncthreads();
    AM_MARK(3);                                                // carrier (or FFT while not FINE) + line fit + NCO correction

    // ---- pass 2: the block's spectra (acquire.c:237-257) -> sync_process_am on the LDS tile --------------------
    am_fold<NT>(sm, win, samperr, sm.theta, sm.step270, sm.step256);
    AM_MARK(4);                                                // pass-2 fold
    am_fft_all<NT>(sm);
    AM_MARK(5);                                                // 32 x FFT-256

    // lower sideband: z = -conj(z); complementary sidebands of the hybrid waveform add coherently (sync.c:616-633)
    for (int id = tid; id < NSYM * AM_IDX_MAX; id += NT) {
        const int n = id / AM_IDX_MAX, i = 1 + id % AM_IDX_MAX;
        float2 &lo = am_bin(sm, -i, n);
        lo = make_float2(-lo.x, lo.y);
        if (!sm.ma3 && i <= 53) { float2 &up = am_bin(sm, i, n); up = make_float2(up.x + lo.x, up.y + lo.y); }
    }
    __syncthreads();
    if constexpr (DUMP) {
        float2 *out = [](float2 *x, float2 *) { return x; }(dump...);
        for (int k = tid; k < NSYM * AM_FFT; k += NT) out[k] = sm.X[k];
    }
    if (tid < 64) {
        const unsigned long long m = __ballot(tid < NSYM && am_bin(sm, 1, tid & 31).y > 0);
        if (tid == 0) sm.refmask = (int)(uint32_t)m;           // bit n = reference-carrier BPSK bit of symbol n
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned d = (unsigned)sm.refmask;
        // the state words of this section in one burst, worked on as values, stored where they change (read through the state at every test they were
        // a chain of dependent L2 round trips: every store in between forces the next read back to memory)
        int sync_state = st.sync_state, cfo_wait = st.cfo_wait, psmi = st.psmi, bc_now = st.bc, rdbi = am.rdbi;
        // fixed part of the reference sequence (find_ref_am / find_block_am needles, sync.c:211-213,242-244)
        const unsigned care23 = 0x60427fu, val23 = 0x600226u;  // positions 0-6, 9, 14, 21, 22; ones at 1, 2, 5, 9, 21, 22
        if (sync_state == SYNC_COARSE && cfo_wait == 0) {
            int off = -1;
            for (int r = 0; r < NSYM && off < 0; r++) {
                const unsigned rot = r ? ((d >> r) | (d << (32 - r))) : d;      // rot bit i = d[(r + i) % 32]
                if ((rot & care23) == val23) off = r;
            }
            if (off > 0) { st.keep_extra = ((NSYM - off) % NSYM) * AM_SYM; st.cfo_wait = 8; }
        } else {
            st.cfo_wait = cfo_wait - 1;
        }
        if (sync_state == SYNC_COARSE) {
            int bc = -1;
            auto bit = [&](int k) { return (d >> k) & 1u; };
            if ((d & care23) == val23
                && !(bit(7) ^ bit(8))
                && !(bit(10) ^ bit(11) ^ bit(12) ^ bit(13))
                && !(bit(15) ^ bit(16) ^ bit(17) ^ bit(18) ^ bit(19) ^ bit(20))
                && !(__popc(d & 0xff800000u) & 1)) {
                bc = (int)((bit(17) << 2) | (bit(18) << 1) | bit(19));
                if (bc == 0) {
                    psmi = (int)((bit(26) << 4) | (bit(27) << 3) | (bit(28) << 2) | (bit(29) << 1) | bit(30));
                    st.psmi = psmi;
                    rdbi = (int)bit(15);
                    am.pli = bit(7); am.hppi = bit(11); am.aabi = bit(12); am.rdbi = rdbi;
                }
            }
            unsigned history = bc == -1 ? 0u : ((am.offset_history << 4) | (unsigned)bc);
            if ((history & 0xffffu) == 0x5670u) {
                bc_now = 0; st.bc = 0;
                sync_state = SYNC_FINE; st.sync_state = SYNC_FINE; st.fine_epoch++;    // input_set_sync_state: EVENT_SYNC payload (input.c:179-185)
                rec.flags |= REC_TO_FINE;
                rec.freq_offset = (float)(((double)st.prev_angle - 2 * M_PI * st.cfo) * 46511.71875 / (2 * M_PI * AM_FFT));
                rec.sis = (uint32_t)((am.pli & 1) | ((am.hppi & 1) << 1) | ((am.aabi & 1) << 2) | ((rdbi & 1) << 3) | 16);
                am.am_errors = 0; am.am_diversity_wait = 4;    // decode_reset (decode.c:563-572)
                history = 0;
            }
            am.offset_history = history;
        }
        sm.fine = sync_state == SYNC_FINE;
        sm.ma3 = psmi == AM_MA3;
        sm.bc_now = bc_now; sm.psmi_now = psmi; sm.rdbi_now = rdbi;
    }
    __syncthreads();
    AM_MARK(6);                                                // sideband combine + reference-sequence decode (one work-item)

    if (sm.fine) {
        const bool ma3 = sm.ma3 != 0;
        const int bc = sm.bc_now;
        // PIDS carriers: normalise by the two training symbols (8 and 24), slice QAM16 (sync.c:661-678)
        if (tid < 2 * NSYM) {
            const int n = tid >> 1, which = tid & 1;
            const int off = which == 0 ? (ma3 ? -27 : 27) : (ma3 ? 27 : 53);
            const float2 t8 = am_bin(sm, off, 8), t24 = am_bin(sm, off, 24);
            const float2 mult = cdivf(make_float2(3.0f, -1.0f), make_float2(t8.x + t24.x, t8.y + t24.y));
            sm.pids_sym[tid] = (uint8_t)sym_qam16(cmulf(am_bin(sm, off, n), mult));
        }
        // per-carrier equaliser taps from the two training cells of each carrier (sync.c:689-714)
        if (tid < 4 * AM_PW) {
            const int part = tid / AM_PW, col = tid % AM_PW;
            const int t1 = (5 + 11 * col) % 32, t2 = (21 + 11 * col) % 32;
            const int pri = ma3 ? 2 : 57, ter = ma3 ? 28 : 2;
            int off; float2 ideal;
            if (part == 0) { off = -(pri + col); ideal = make_float2(5.0f, -5.0f); }
            else if (part == 1) { off = pri + col; ideal = make_float2(5.0f, -5.0f); }
            else if (part == 2) { off = 28 + col; ideal = ma3 ? make_float2(5.0f, -5.0f) : make_float2(3.0f, -1.0f); }
            else { off = ma3 ? -(ter + col) : ter + col; ideal = ma3 ? make_float2(5.0f, -5.0f) : make_float2(-1.0f, 1.0f); }
            const float2 a = am_bin(sm, off, t1), b2 = am_bin(sm, off, t2);
            const float2 m = cdivf(ideal, make_float2(a.x + b2.x, a.y + b2.y));
            sm.mult[part][col] = m;
            if (part < 2) sm.marg[part][col] = ref_atan2f(m.y, m.x);
        }
        __syncthreads();
        if constexpr (DUMP) {
            float2 *out = [](float2 *, float2 *m) { return m; }(dump...);
            for (int k = tid; k < 4 * AM_PW; k += NT) out[k] = sm.mult[k / AM_PW][k % AM_PW];
        }
        AM_MARK(7);                                            // PIDS carriers + equaliser taps
        if (tid == 0) {
            float se = 0;
            for (int col = 1; col < AM_PW; col++) {
                se += half_turn_diff(sm.marg[0][col], sm.marg[0][col - 1]);
                se += half_turn_diff(sm.marg[1][col], sm.marg[1][col - 1]);
            }
            se = (float)((double)(se / (2 * (AM_PW - 1)) * AM_FFT) / (2 * M_PI));
            st.samperr = (int)roundf(se);
        }
        // equalise and slice the four partitions: hard symbols of this block go to the frame matrices (decode.c:439-449)
        uint8_t *symbase = db.am_sym + (size_t)s * 4 * AM_SYMS;
        for (int id = tid; id < 4 * NSYM * AM_PW; id += NT) {
            const int part = id / (NSYM * AM_PW), r = id % (NSYM * AM_PW), n = r / AM_PW, col = r % AM_PW;
            const int pri = ma3 ? 2 : 57, ter = ma3 ? 28 : 2;
            int off;
            if (part == 0) off = -(pri + col); else if (part == 1) off = pri + col; else if (part == 2) off = 28 + col;
            else off = ma3 ? -(ter + col) : ter + col;
            const float2 v = cmulf(am_bin(sm, off, n), sm.mult[part][col]);
            unsigned code;
            if (part < 2 || ma3) code = sym_qam64(v);
            else if (part == 2) code = sym_qam16(v);
            else code = sym_qpsk(v);
            symbase[(size_t)part * AM_SYMS + bc * (NSYM * AM_PW) + r] = (uint8_t)code;
        }
        __syncthreads();
        AM_MARK(8);                                            // timing estimate + equalise / slice
        // PIDS: bit gather (decode.c:476-501), K=9 E2 decode, descramble
        if (tid < 120) {
            const int n = tid, p = n % 4;
            int k = (n + (n / 60) + 11) % 30, row = (11 * (k + (k / 15)) + 3) % 32;
            const int il = (sm.pids_sym[row * 2] >> p) & 1;
            k = (n + (n / 60)) % 30; row = (11 * (k + (k / 15)) + 3) % 32;
            const int iu = (sm.pids_sym[row * 2 + 1] >> p) & 1;
            const int i = n / 12, j = n % 12;
            const int il_pos[12] = { 0, 1, 12, 13, 6, 5, 18, 17, 11, 7, 23, 19 };      // decode.c:63-64
            const int iu_pos[12] = { 2, 4, 14, 16, 3, 8, 15, 20, 9, 10, 21, 22 };
            const bool pids1_disabled = (sm.psmi_now == 1) && sm.rdbi_now;
            sm.pids_coded[i * 24 + il_pos[j]] = pids1_disabled ? 0 : (il ? 1 : -1);
            sm.pids_coded[i * 24 + iu_pos[j]] = iu ? 1 : -1;
        }
        __syncthreads();
        if (pipeline) {
            // window pipeline: the 144-step PIDS trellis leaves the step chain -- stage its input for k_am_decode
            int8_t *stage = db.am_pids_stage + (((size_t)s * NWIN + parity) * 8 + slot) * (3 * PIDS_LEN);
            if (tid < 3 * PIDS_LEN) stage[tid] = sm.pids_coded[tid];
            if (tid == 0) db.am_pids_rec[((size_t)s * NWIN + parity) * 8 + slot] = st.nblocks % db.rec_cap;
        } else {
            K9Smem &k9 = *(K9Smem *)sm.X;
            unsigned long long *pids_dec = (unsigned long long *)((uint8_t *)sm.X + sizeof(K9Smem));
            viterbi_k9_block(sm.pids_coded, PIDS_LEN, GEN_E2_0, GEN_E2_1, GEN_E2_2, pids_dec, sm.pids_out, k9);
        }
        if (tid == 0) {
            if (!pipeline) {
                // (CRC over a local copy: on the record itself every one of its 80 bits was a round trip to global memory)
                const uint32_t p[3] = { sm.pids_out[0] ^ tb.scr_pids[0], sm.pids_out[1] ^ tb.scr_pids[1], (sm.pids_out[2] ^ tb.scr_pids[2]) & 0xffffu };
                rec.pids[0] = p[0]; rec.pids[1] = p[1]; rec.pids[2] = p[2];
                rec.flags |= pids_crc_ok(p) ? (uint32_t)REC_PIDS_CRC : 0u;
            }
            rec.flags |= REC_PIDS;
            rec.bc_decoded = bc;
            // hand this block to the P1 / P3 decoders (decode_process_p1_p3_am runs next, in k_am_viterbi)
            am.dec_bc = bc; am.dec_record = st.nblocks % db.rec_cap; am.dec_rdbi = am.rdbi; am.dec_psmi = st.psmi;
            if (bc == 0) {
                am.am_errors = 0;
                if (am.am_diversity_wait == 0) { am.frame_slot = am.next_slot; am.vit_parity = am.next_job; }
            }
            if (pipeline && am.am_diversity_wait == 0) {
                // the frame's decodes run (or ran) on a decode stream from the trellis inputs of the previous L1 frame:
                // this block only announces what decode_process_p1_p3_am delivers here (decode.c:507-554)
                rec.flags |= REC_P1 | ((bc == 7 && !am.rdbi) ? (uint32_t)REC_P3 : 0u);
                rec.p1_slot = am.frame_slot;
                if (db.am_ckpt) {
                    // frame_process judges this PDU's first header inside this very block (frame.c:535-540).  If the deferred
                    // decode has already filed a failure, apply it now; else run on and let k_rollback_am rewind to the
                    // checkpoint k_am_interleave takes at the end of this step (k_replay.hip)
                    AmJob &dj = db.am_job[(size_t)s * NWIN + am.vit_parity];
                    dj.deliver_abs[bc] = st.nblocks;
                    sm.deliver = bc;
                    if (atomicAdd(&dj.verdict[bc], 0) == 2) { dj.verdict[bc] = 3; st.sync_state = SYNC_NONE; rec.flags |= REC_LOST_SYNC; }
                }
            }
            st.bc = (bc + 1) % 8;
        }
    }

    AM_MARK(9);                                                // PIDS gather / stage + frame hand-off (one work-item)
    // ---- tail of acquire_process (acquire.c:259-262) + record -------------------------------------------------------
    // Two work-items of different waves share it, as in k_sync: the NCO phase with its double-precision cosine / sine (a diagnostic of the record) on
    // one, the FIFO position and the record on the other with its state loads issued together (a load behind every store of the other kind cost an
    // L2 round trip apiece).
    if (tid == 64) {
        double th = sm.theta + sm.dtheta * (double)(NSYM * AM_SYM);
        th -= 2 * M_PI * rint(th / (2 * M_PI));
        st.theta = th;
        rec.phase_re = (float)cos(th); rec.phase_im = (float)sin(th);
    }
    if (tid == 0) {
        const int keep_extra = st.keep_extra, state = st.sync_state, cfo = st.cfo, bc_now = st.bc, psmi = st.psmi, cfo_wait = st.cfo_wait, next_samperr = st.samperr, nblocks = st.nblocks;
        const long long rd = st.rd;
        const float prev_angle = st.prev_angle, next_angle = st.angle;   // (sync_t.angle: zero in this mode unless a reset carried it over from an FM session)
        const int keep = AM_SYM + (AM_SYM / 2 - samperr) + keep_extra;
        st.keep_extra = 0;
        st.rd = rd + (AM_WIN - keep);
        rec.state_after = state; rec.samperr = samperr; rec.cfo = cfo; rec.keep = keep; rec.bc = bc_now;
        rec.psmi = psmi; rec.cfo_wait = cfo_wait; rec.next_samperr = next_samperr;
        rec.prev_angle = prev_angle; rec.next_angle = next_angle;
        st.nblocks = nblocks + 1;
    }
    AM_MARK(10);                                               // tail
    if (db.am_ckpt) {                                          // block-uniform: window pipeline with the on-device L2 feedback
        // Replay checkpoint of a block that delivered a P1 PDU (k_replay.hip): the state as of now.  For block 7 the
        // de-interleaver's bookkeeping (k_am_interleave, next) still belongs to the block: k_rollback_am adds it on restore.
        __threadfence_block();
        __syncthreads();
        const int j = sm.deliver;
        if (j >= 0) {
            AmCkpt &ck = db.am_ckpt[((size_t)s * NWIN + am.vit_parity) * 8 + j];
            const uint32_t *a = (const uint32_t *)&st, *b = (const uint32_t *)&am;
            uint32_t *da = (uint32_t *)&ck.st, *dbp = (uint32_t *)&ck.am;
            for (int k = tid; k < (int)(sizeof(StreamState) / 4); k += NT) da[k] = a[k];
            for (int k = tid; k < (int)(sizeof(AmStream) / 4); k += NT) dbp[k] = b[k];
        }
    }
}

// ---- after block 7: BER of the frame just decoded, then interleaver_ma1 for the frame just received -------------
// Output-centric and table-driven: every depunctured trellis input looks up which bit of which hard-symbol matrix it is
// (DevTables::am_deint_*, built from decode.c:66-231 by engine.hip), the main (m*) bits pass through the 3-frame
// diversity delay lines -- a 3-slot ring with one cell per trellis input, whose oldest slot is read and refilled in place by the
// same work-item (consecutive work-items, consecutive bytes).
// Four inputs per work-item and trip: the table entries AND the delay cells (their address does not depend on the entry -- a cell
// that is not a delayed input's is simply not used) are requested together, then the LDS look-ups, then the stores; one input per
// trip left the kernel waiting for three dependent round trips per input.
__device__ inline void am_deint_span(const uint32_t *tab, int n, const uint8_t *sym, uint8_t *q, int8_t *v, int i0, int step)
{
    for (int i = i0; i < n; i += 4 * step) {
        uint32_t e[4]; uint8_t old[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int k = i + u * step;
            e[u] = k < n ? tab[k] : AMT_PUNCT;
            old[u] = k < n ? q[k] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int k = i + u * step;
            if (k >= n) break;
            int8_t out = 0;
            if (!(e[u] & AMT_PUNCT)) {
                const uint8_t *m = sym + (size_t)((e[u] >> 16) & 3u) * AM_SYMS;
                int bit = (m[e[u] & 0x1fffu] >> ((e[u] >> 13) & 7u)) & 1;
                if (e[u] & AMT_DELAYED) { q[k] = (uint8_t)bit; bit = old[u]; }
                out = bit ? 1 : -1;
            }
            v[k] = out;
        }
    }
}

// The 162 000 (MA1) / 180 000 (MA3) trellis inputs of an L1 frame are independent table look-ups (every cell of the diversity delay
// lines is visited by exactly one of them), so the frame is cut into AM_IL_PARTS slices, one workgroup each: with diverse streams an
// eighth of the batch finishes an L1 frame in any one step, and one workgroup per stream left 7 of 8 CUs idle for the 90 us such a
// step then took.  The bookkeeping that ends the frame -- delay-line head, ring slot and decode job of the next frame -- is done by
// the slice that finishes last (AmStream::il_done counts them).
constexpr int AM_IL_PARTS = 32;
constexpr int AM_IL_THREADS = 256;          // 4-wave workgroups find room between the decode waves; 16-wave ones wait for it

__device__ inline void am_deinterleave_slice(const DevTables &tb, const DevBuffers &db, int s, int parity, int part)
{
    AmStream &am = db.am[s];
    const bool ma3 = am.dec_psmi == AM_MA3;
    const int tid = threadIdx.x;
    const int vslot = parity < 0 ? 0 : parity;                 // window pipeline: one set of trellis inputs per window in flight
    if (part == 0 && tid == 0 && parity < 0 && am.am_diversity_wait == 0) {
        db.records[(size_t)s * db.rec_cap + am.dec_record].ber = (float)am.am_errors / (float)am_frame_coded_bits(am.dec_psmi, am.dec_rdbi);
    }
    // the frame's four hard-symbol matrices (25.6 KB) are gathered from byte by byte in interleaver order: stage them in LDS
    // first (the scattered byte loads were what the kernel waited for)
    __shared__ __attribute__((aligned(16))) uint8_t sym[4 * AM_SYMS];   // [pl, pu, s, t][8 blocks][32][25]
    static_assert((4 * AM_SYMS) % 16 == 0, "symbol matrices are copied in 16-byte pieces");
    {
        const uint4 *src = (const uint4 *)(db.am_sym + (size_t)s * 4 * AM_SYMS);
        for (int k = tid; k < 4 * AM_SYMS / 16; k += AM_IL_THREADS) ((uint4 *)sym)[k] = src[k];
    }
    __syncthreads();
    uint8_t *q1 = db.am_q + ((size_t)s * 3 + am.q_head) * 2 * AM_VIT, *q3 = q1 + AM_VIT;   // the oldest of the three frames in the delay lines
    int8_t *v1 = db.am_vit + ((size_t)s * db.am_nvit + vslot) * 2 * AM_VIT, *v3 = v1 + AM_VIT;
    const int i0 = part * AM_IL_THREADS + tid, step = AM_IL_THREADS * AM_IL_PARTS;
    am_deint_span(tb.am_deint_p1, AM_VIT, sym, q1, v1, i0, step);
    if (!ma3) am_deint_span(tb.am_deint_p3_ma1, 3 * AM_P3_LEN_MA1, sym, q3, v3, i0, step);
    else am_deint_span(tb.am_deint_p3_ma3, AM_VIT, sym, q3, v3, i0, step);
}

// after EVERY slice of the frame: advance the delay lines, reserve the ring slot and the decode job of the next L1 frame
__device__ inline void am_deinterleave_commit(const DevBuffers &db, int s, int parity, int window)
{
    AmStream &am = db.am[s];
    am.q_head = (am.q_head + 1) % 3;
    if (am.am_diversity_wait > 0) am.am_diversity_wait--;
    if (am.am_diversity_wait == 0) {
        // the next L1 frame delivers what these trellis inputs decode to: reserve its ring slot now
        StreamState &stw = db.state[s];
        am.next_slot = stw.p1_count % db.p1_slots; stw.p1_count++;
        if (parity >= 0) {
            AmJob &job = db.am_job[(size_t)s * NWIN + parity];
            job.slot = am.next_slot; job.psmi = am.dec_psmi; job.rdbi = am.dec_rdbi; job.errors = 0; job.done = 0; job.pad = 0; job.epoch = stw.fine_epoch;
            for (int j = 0; j < 8; j++) { job.verdict[j] = 0; job.deliver_abs[j] = -1; }
            job.window = window;
            am.next_job = parity;
            job.valid = 1;
        }
    }
}

__global__ __launch_bounds__(AM_IL_THREADS) void k_am_interleave(DevTables tb, DevBuffers db, const int *ids, int parity, int window)
{
    wave_set_priority_high();
    const int s = stream_of(ids, blockIdx.y);
    const StreamState &st = db.state[s];
    AmStream &am = db.am[s];
    if (!st.active || am.dec_bc != 7) return;                  // block-uniform
    am_deinterleave_slice(tb, db, s, parity, (int)blockIdx.x);
    // the slice that finishes last commits the frame: every other slice has read q_head / dec_* by then (their loads completed
    // before the barrier below; no fence -- an agent-scope fence per work-item writes back and invalidates L2 two million times a
    // launch, measured: the pass 98 -> 143 ms)
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(&am.il_done, 1u) == (unsigned)(AM_IL_PARTS - 1)) {
        am.il_done = 0;
        am_deinterleave_commit(db, s, parity, window);
    }
}

// (per device: the attribute belongs to the function as loaded on the current device -- one process may drive several, include/nrsc5hip.h)
static void am_block_attributes()
{
    static std::atomic<bool> attr_set[64];
    int dev = 0; (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev].load(std::memory_order_acquire)) {      // (a device index beyond the table: set it on every launch rather than never)
        (void)hipFuncSetAttribute((const void *)k_am_block<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(AmBlockSmem));
        (void)hipFuncSetAttribute((const void *)k_am_block<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(AmBlockSmem));
        (void)hipFuncSetAttribute((const void *)k_am_block<512, true, float2 *, float2 *>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(AmBlockSmem));
        (void)hipFuncSetAttribute((const void *)k_am_block<256, true, float2 *, float2 *>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(AmBlockSmem));
        if (dev >= 0 && dev < 64) attr_set[dev].store(true, std::memory_order_release);
    }
}

// k_am_block alone, for the stage hook (nrsc5hip_stage_am_block): the launch shapes of launch_am_step, without the decode and interleave launches behind them.
// dump_x / dump_mult non-null: the dumping instantiation
void launch_stage_am_block(const DevTables &tb, const DevBuffers &db, int pipeline, float2 *dump_x, float2 *dump_mult, hipStream_t st)
{
    am_block_attributes();
    const int *ids = nullptr;
    if (dump_x && dump_mult) {
        if (pipeline) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_am_block<512, true, float2 *, float2 *>), dim3(1), dim3(512), sizeof(AmBlockSmem), st, tb, db, ids, 1, 0, 0, dump_x, dump_mult);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_am_block<256, true, float2 *, float2 *>), dim3(1), dim3(256), sizeof(AmBlockSmem), st, tb, db, ids, 0, -1, 0, dump_x, dump_mult);
    } else {
        if (pipeline) hipLaunchKernelGGL(k_am_block<512>, dim3(1), dim3(512), sizeof(AmBlockSmem), st, tb, db, ids, 1, 0, 0);
        else hipLaunchKernelGGL(k_am_block<256>, dim3(1), dim3(256), sizeof(AmBlockSmem), st, tb, db, ids, 0, -1, 0);
    }
}

void launch_am_step(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, hipStream_t st, int l2_feedback, int pipeline_parity, int slot, int window)
{
    am_block_attributes();
    if (pipeline_parity >= 0) hipLaunchKernelGGL(k_am_block<512>, dim3(nstreams), dim3(512), sizeof(AmBlockSmem), st, tb, db, stream_ids, 1, pipeline_parity, slot);
    else hipLaunchKernelGGL(k_am_block<256>, dim3(nstreams), dim3(256), sizeof(AmBlockSmem), st, tb, db, stream_ids, 0, pipeline_parity, slot);
    if (pipeline_parity < 0) launch_am_decode_in_order(tb, db, nstreams, stream_ids, l2_feedback, st);
    launch_am_interleave(tb, db, nstreams, stream_ids, pipeline_parity, window, st);
}

void launch_am_interleave(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int window, hipStream_t st)
{
    hipLaunchKernelGGL(k_am_interleave, dim3(AM_IL_PARTS, nstreams), dim3(AM_IL_THREADS), 0, st, tb, db, stream_ids, parity, window);
}

}  // namespace nrsc5
