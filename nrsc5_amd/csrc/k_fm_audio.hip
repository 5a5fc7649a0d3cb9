// Analog FM audio of a station's 744 187.5 S/s cs16 stream (include/nrsc5hip.h, "analog FM audio"; the definition: DESIGN.md (o)).
//
// Every quantity is a function of absolute sample indices (x[n] = 0 for n < 0), no recurrence anywhere: any chunking gives the same bytes.
//   k_fm_front  one workgroup = FT consecutive Fs1 outputs of one channel.  The cs16 span (new input and kept history) is staged in LDS as
//               float2 from 4-byte loads, every work-item sums one z[m] = sum_i hA[i] x[2 m - i] (the tile one more than it emits), and the
//               discriminator d[m] = atan2(z[m] conj z[m - 1]) goes to the channel's d buffer as float32; with the carrier measurement enabled
//               also r[m] = |z[m]|^2 (k_fm_carrier.hip).
//   k_fm_pilot  one wave = one complete pilot block: p[j] = sum d[m] exp(-j phi19(m)) in a fixed order (9 terms per lane, then a butterfly),
//               so the sum does not depend on which push completed the block.  No atomics.
//   k_fm_audio  one workgroup = one pilot block = 64 audio outputs.  Every wave forms the smoothed pilot (33 block sums, a butterfly), the d span
//               and the difference path 2 eq(d) sub go to LDS, and the block's 4 waves each sum a quarter of the taps of the 64 outputs for
//               both paths from one table load; wave 0 adds the quarters in order, rounds, clamps and writes L, R.  Steered by reception
//               (k_fm_audio<true>) every wave also forms the windowed carrier moments of blocks j - 1 and j from k_fm_carrier's
//               triples and from them blend, high-cut and mute; the tap loop reads a second, narrow table only in a block whose high-cut is
//               live, and wave 0 mixes.
//   k_fm_keep   what the next call needs: the tail of d, of the block sums and of the input (as k_chan_history).
// The pilot phase (608 m mod 11907) indexes a table of 11907 (cos, sin) pairs computed in double on the host: exact to float32 rounding,
// the same bits on the device and in the CPU twin.
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>
#include "fm_audio.h"
#include "fastmath.h"

namespace nrsc5 {
namespace fm {
namespace {

__device__ __forceinline__ float2 unpack_cs16(int v) { return make_float2((float)(short)(v & 0xffff), (float)(short)(v >> 16)); }

// sample at absolute index n of channel ch, n < n0 + n_in
__device__ __forceinline__ int load_x(const FrontArgs &a, const int *in32, const int *hist, long long n)
{
    if (n >= a.n0) return n < a.n0 + a.n_in ? in32[n - a.n0] : 0;
    const long long h = n - (a.n0 - HIST);
    return h >= 0 ? hist[h] : 0;                              // (n >= 0 never reaches back further; n < 0 reads the zeros the history starts with)
}

// WITH_R: also r[m] = |z[m]|^2 for the carrier measurement (k_fm_carrier.hip).  A template, not a test of the pointer: the instantiation without
// it is the kernel as it was, instruction for instruction
template <bool WITH_R> __global__ __launch_bounds__(256) void k_fm_front(FrontArgs a)
{
    HIP_DYNAMIC_SHARED(float2, sm);
    float2 *xs = sm, *zs = sm + (2 * FT + TA);
    const int ch = blockIdx.y;
    const long long mt0 = a.m0 + (long long)blockIdx.x * FT;
    const long long left = a.m0 + a.m_count - mt0;
    const int cnt = left < FT ? (int)left : FT;
    if (cnt <= 0) return;
    const long long n_lo = 2 * (mt0 - 1) - (TA - 1);          // x index of xs[0]; xs[2 q + TA - 1 - i] = x[2 (mt0 - 1 + q) - i]
    const int span = 2 * cnt + TA;
    const int *in32 = (const int *)(a.in + (long long)ch * a.in_stride);
    const int *hist = a.hist + (long long)ch * HIST;
    for (int k = threadIdx.x; k < span; k += blockDim.x) {
        const long long n = n_lo + k;
        xs[k] = n < 0 ? make_float2(0.0f, 0.0f) : unpack_cs16(load_x(a, in32, hist, n));
    }
    __syncthreads();
    for (int q = threadIdx.x; q <= cnt; q += blockDim.x) {    // z[mt0 - 1 + q]
        const float2 *v = xs + 2 * q + TA - 1;
        float re = 0.0f, im = 0.0f;
#pragma unroll 16                                            // 16 taps per scalar load; unrolled whole, the 112 taps spill out of the SGPRs
        for (int i = 0; i < TA; i++) {
            const float t = a.ha[i];
            const float2 x = v[-i];
            re = fmaf(x.x, t, re); im = fmaf(x.y, t, im);
        }
        zs[q] = make_float2(re, im);
    }
    __syncthreads();
    const int q = threadIdx.x + 1;
    if (q <= cnt) {
        const long long m = mt0 - 1 + q;
        const float2 z = zs[q], zp = zs[q - 1];
        const float re = fmaf(z.x, zp.x, z.y * zp.y), im = fmaf(z.y, zp.x, -(z.x * zp.y));      // z conj(zp)
        float d = 0.0f;
        if (m > 0 && !(re == 0.0f && im == 0.0f)) d = ref_atan2f(im, re) * DEV_SCALE;
        a.d[(long long)ch * a.d_stride + (m - a.d_base)] = d;
        if (WITH_R) a.r[(long long)ch * a.r_stride + (m - a.r_base)] = fmaf(z.x, z.x, z.y * z.y);
    }
}

__device__ __forceinline__ float wave_sum(float v)
{
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);  // a + b == b + a: every lane ends with the same bits
    return v;
}

__global__ __launch_bounds__(64) void k_fm_pilot(PilotArgs a)
{
    const int ch = blockIdx.y;
    const long long j = a.j0 + blockIdx.x;
    const float *d = a.d + (long long)ch * a.d_stride + ((long long)BLOCK * j - a.d_base);
    float re = 0.0f, im = 0.0f;
    for (int mi = threadIdx.x; mi < BLOCK; mi += 64) {
        const long long m = (long long)BLOCK * j + mi;
        const float2 t = a.cs[(int)((PILOT_NUM * m) % PILOT_DEN)];
        const float v = d[mi];
        re = fmaf(v, t.x, re); im = fmaf(-v, t.y, im);       // d exp(-j phi)
    }
    re = wave_sum(re); im = wave_sum(im);
    if (threadIdx.x == 0) a.p[(long long)ch * a.p_stride + (j - a.p_base)] = make_float2(re, im);
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// reception steering: the quality q of audio block jq from k_fm_carrier's block triples under the pilot's window, in
// k_fm_carrier_report's arithmetic (lane w + W holds term w, each product in double, the xor butterfly): the same bits in every wave.  c is the
// window's weight over the blocks that exist, not the constant 17: the first 16 blocks of a session lose the part in front of the stream
__device__ __forceinline__ double steer_quality(const SteeredAudioArgs &a, int ch, long long jq, int lane)
{
    double w2 = 0.0, w4 = 0.0, c = 0.0;
    const long long jb = jq + lane - W;
    if (lane <= 2 * W && jb >= 0) {
        const double *v = a.t + 3 * ((long long)ch * a.t_stride + (jb - a.t_base));
        const double w = (double)a.win[lane];
        w2 = v[0] * w; w4 = v[1] * w; c = w;
    }
    w2 = wave_sum(w2); w4 = wave_sum(w4); c = wave_sum(c);
    if (!(w2 > 0.0)) return 0.0;
    const double kappa = w4 * (540.0 * c) / (w2 * w2);
    return fmin(1.0, fmax(0.0, 2.0 - kappa));
}

__device__ __forceinline__ float steer_ramp(float q, float lo, float inv) { return fminf(1.0f, fmaxf(0.0f, (q - lo) * inv)); }

// the three factors (b, h, g) of a block of quality q; a control that is off has factor 1
__device__ __forceinline__ void steer_factors(const SteerRamps &r, double q, float &b, float &h, float &g)
{
    const float qf = (float)q;
    b = (r.controls & NRSC5HIP_FM_STEER_BLEND) ? steer_ramp(qf, r.blend_lo, r.blend_inv) : 1.0f;
    h = (r.controls & NRSC5HIP_FM_STEER_HIGHCUT) ? steer_ramp(qf, r.highcut_lo, r.highcut_inv) : 1.0f;
    g = (r.controls & NRSC5HIP_FM_STEER_MUTE) ? fmaf(steer_ramp(qf, r.mute_lo, r.mute_inv), 1.0f - r.mute_floor, r.mute_floor) : 1.0f;   // exactly 1 at the top
}

// STEER: the audio steered by reception.  A template: the instantiation without it is the kernel as it was, instruction for
// instruction
template <bool STEER> __global__ __launch_bounds__(256) void k_fm_audio(std::conditional_t<STEER, SteeredAudioArgs, AudioArgs> a)
{
    HIP_DYNAMIC_SHARED(float, lds);
    const int tb = a.tb, ch = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    float *ds = lds;                                         // [tb + 542]: d[mlo ..], mlo = 540 j - tb - 1
    float *dd = lds + (tb + 542);                            // [tb + 540]: the difference path at m = mlo + 1 ..
    float *part = dd + (tb + 540);                           // [4][64][2], steered [4][4][64]
    const long long j = a.j0 + blockIdx.x;
    const long long mlo = (long long)BLOCK * j - tb - 1;

    // the smoothed pilot: the same loads, the same order in every wave
    float pr = 0.0f, pi = 0.0f;
    if (lane <= 2 * W) {
        const long long jb = j + lane - W;
        if (jb >= 0) {
            const float2 v = a.p[(long long)ch * a.p_stride + (jb - a.p_base)];
            const float w = a.win[lane];
            pr = v.x * w; pi = v.y * w;
        }
    }
    pr = wave_sum(pr); pi = wave_sum(pi);
    const float mag = sqrtf(pr * pr + pi * pi);
    const float level = 2.0f * mag / (float)BLOCK / a.wsum;
    const bool stereo = level >= a.pilot_min;

    // steered: the factors at the end of block j - 1 (c0; block 0 starts at its own) and of block j (c1), the same bits in every wave; `narrow`
    // and `diff` are uniform over the block
    float q1 = 0.0f, b0 = 1.0f, b1 = 1.0f, h0 = 1.0f, h1 = 1.0f, g0 = 1.0f, g1 = 1.0f;
    bool narrow = false, diff = stereo;
    if constexpr (STEER) {
        const double qa = steer_quality(a, ch, j > 0 ? j - 1 : 0, lane), qb = steer_quality(a, ch, j, lane);
        steer_factors(a.ramps, qa, b0, h0, g0);
        steer_factors(a.ramps, qb, b1, h1, g1);
        q1 = (float)qb;
        narrow = !(h0 == 1.0f && h1 == 1.0f);                // both ends wide: the narrow sums are skipped
        diff = stereo && !(b0 == 0.0f && b1 == 0.0f);        // both ends mono: the difference path is skipped, L == R
    }

    const float *d = a.d + (long long)ch * a.d_stride;
    for (int i = tid; i < tb + 542; i += 256) {
        const long long m = mlo + i;
        ds[i] = m >= 0 ? d[m - a.d_base] : 0.0f;
    }
    __syncthreads();
    if (diff) {
        const float ur = pr / mag, ui = pi / mag;            // exp(j 2 theta) = -(p / |p|)^2: the pilot is a sine
        const float c2 = -(ur * ur - ui * ui), s2 = -(2.0f * ur * ui);
        for (int i = tid; i < tb + 540; i += 256) {
            const long long m = mlo + 1 + i;
            float v = 0.0f;
            if (m >= 0) {
                const float2 t = a.cs[(int)((2 * PILOT_NUM * m) % PILOT_DEN)];
                const float sub = t.y * c2 + t.x * s2;       // sin(2 phi19(m) + 2 theta)
                v = 2.0f * (a.aq * ds[i] + a.bq * ds[i + 1] + a.aq * ds[i + 2]) * sub;
            }
            dd[i] = v;
        }
    }
    __syncthreads();

    const int qtr = tid >> 6;
    const long long k = (long long)BLOCK_OUT * j + lane;
    const long long t16 = (long long)T_NUM * k;
    const int base = (int)((t16 >> 4) - mlo), ph = (int)(t16 & 15);
    const int tq = (tb + 3) / 4, j0 = qtr * tq, j1 = min(tb, j0 + tq);
    const float *tab = a.tab + ph;
    float s = 0.0f, dl = 0.0f, sn = 0.0f, dn = 0.0f;
    const float *tabn = tab;
    if constexpr (STEER) tabn = a.tab_n + ph;
    if (STEER && narrow) {                                   // both tables from the same two LDS reads
        if (diff) {
            for (int jj = j0; jj < j1; jj++) {
                const float t = tab[jj * PHASES], tn = tabn[jj * PHASES], x = ds[base - jj], y = dd[base - 1 - jj];
                s = fmaf(t, x, s); dl = fmaf(t, y, dl);
                sn = fmaf(tn, x, sn); dn = fmaf(tn, y, dn);
            }
        } else {
            for (int jj = j0; jj < j1; jj++) {
                const float x = ds[base - jj];
                s = fmaf(tab[jj * PHASES], x, s); sn = fmaf(tabn[jj * PHASES], x, sn);
            }
        }
    } else if (diff) {
        for (int jj = j0; jj < j1; jj++) {
            const float t = tab[jj * PHASES];
            s = fmaf(t, ds[base - jj], s);
            dl = fmaf(t, dd[base - 1 - jj], dl);
        }
    } else {
        for (int jj = j0; jj < j1; jj++) s = fmaf(tab[jj * PHASES], ds[base - jj], s);
    }
    if (STEER) {                                             // [4 sums][4 quarters][64]
        part[qtr * 64 + lane] = s; part[(4 + qtr) * 64 + lane] = dl; part[(8 + qtr) * 64 + lane] = sn; part[(12 + qtr) * 64 + lane] = dn;
    } else {
        part[(qtr * 64 + lane) * 2] = s; part[(qtr * 64 + lane) * 2 + 1] = dl;
    }
    __syncthreads();
    if (tid < 64) {
        float S, D;
        if (STEER) {
            float4 v = make_float4(part[lane], part[256 + lane], part[512 + lane], part[768 + lane]);      // (Sw, Dw, Sn, Dn), the quarters in order
            for (int q = 1; q < 4; q++) { v.x += part[q * 64 + lane]; v.y += part[(4 + q) * 64 + lane]; v.z += part[(8 + q) * 64 + lane]; v.w += part[(12 + q) * 64 + lane]; }
            // the controls move linearly from block j - 1's value to block j's; with h = b = g = 1 at both ends every operation here is a
            // multiplication by 1 or an fma with weight 0: the bytes of the unsteered kernel
            const float frac = (float)(lane + 1) / 64.0f;
            const float b = fmaf(b1 - b0, frac, b0), h = fmaf(h1 - h0, frac, h0), gm = fmaf(g1 - g0, frac, g0);
            const float Sp = fmaf(h, v.x, (1.0f - h) * v.z), Dp = fmaf(h, v.y, (1.0f - h) * v.w);
            S = (Sp + b * Dp) * gm; D = (Sp - b * Dp) * gm;
        } else {
            S = part[lane * 2]; D = part[lane * 2 + 1];
            for (int q = 1; q < 4; q++) { S += part[(q * 64 + lane) * 2]; D += part[(q * 64 + lane) * 2 + 1]; }
        }
        const float g = a.scale[ch];
        float yl, yr;
        if (STEER) { yl = rintf(S * g); yr = rintf(D * g); }    // S and D hold L and R here
        else { yl = rintf((S + D) * g); yr = rintf((S - D) * g); }
        int cl = 0, cr = 0;
        if (yl > 32767.0f) { yl = 32767.0f; cl = 1; } else if (yl < -32768.0f) { yl = -32768.0f; cl = 1; }
        if (yr > 32767.0f) { yr = 32767.0f; cr = 1; } else if (yr < -32768.0f) { yr = -32768.0f; cr = 1; }
        const unsigned long long bl = __ballot(cl), br = __ballot(cr);
        int16_t *o = a.out + (long long)ch * a.out_stride + 2 * (k - a.k0);
        o[0] = (int16_t)(int)yl; o[1] = (int16_t)(int)yr;
        if (tid == 0) {
            if (bl) atomicAdd(a.clips + 2 * ch, (unsigned long long)__popcll(bl));
            if (br) atomicAdd(a.clips + 2 * ch + 1, (unsigned long long)__popcll(br));
            if (blockIdx.x == gridDim.x - 1) { a.pilot[2 * ch] = level; a.pilot[2 * ch + 1] = stereo ? 1.0f : 0.0f; }
            if constexpr (STEER) {
                if (a.steer_every) a.steer[(long long)ch * a.steer_stride + blockIdx.x] = make_float4(q1, b1, h1, g1);
                else if (blockIdx.x == gridDim.x - 1) a.steer[(long long)ch * a.steer_stride] = make_float4(q1, b1, h1, g1);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_fm_keep(KeepArgs a)
{
    const int ch = blockIdx.y;
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    for (long long i = i0; i < a.d_count; i += step) a.d_new[ch * a.d_stride + i] = a.d_old[ch * a.d_stride + i + a.d_shift];
    for (long long i = i0; i < a.p_count; i += step) a.p_new[ch * a.p_stride + i] = a.p_old[ch * a.p_stride + i + a.p_shift];
    if (i0 < HIST) {                                         // absolute samples [n1 - HIST, n1), n1 = n0 + n_in
        const long long n = a.n0 + a.n_in - HIST + i0;
        int v;
        if (n >= a.n0) v = ((const int *)(a.in + (long long)ch * a.in_stride))[n - a.n0];
        else v = a.hist_old[ch * HIST + (n - (a.n0 - HIST))];
        a.hist_new[ch * HIST + i0] = v;
    }
}

}  // namespace

void launch_front(hipStream_t s, int tiles, int nchan, const FrontArgs &a)
{
    count_launch();
    const size_t lds = sizeof(float2) * (2 * FT + TA + FT + 1);
    if (a.r) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fm_front<true>), dim3(tiles, nchan), dim3(256), lds, s, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fm_front<false>), dim3(tiles, nchan), dim3(256), lds, s, a);
}

void launch_pilot(hipStream_t s, int blocks, int nchan, const PilotArgs &a)
{
    count_launch();
    hipLaunchKernelGGL(k_fm_pilot, dim3(blocks, nchan), dim3(64), 0, s, a);
}

void launch_audio(hipStream_t s, int blocks, int nchan, const AudioArgs &a)
{
    count_launch();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fm_audio<false>), dim3(blocks, nchan), dim3(256), sizeof(float) * (2 * a.tb + 542 + 540 + 512), s, a);
}

void launch_audio_steered(hipStream_t s, int blocks, int nchan, const SteeredAudioArgs &a)
{
    count_launch();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fm_audio<true>), dim3(blocks, nchan), dim3(256), sizeof(float) * (2 * a.tb + 542 + 540 + 1024), s, a);
}

void launch_keep(hipStream_t s, int nchan, const KeepArgs &a)
{
    count_launch();
    long long n = a.d_count > a.p_count ? a.d_count : a.p_count;
    if (n < HIST) n = HIST;
    long long blocks = (n + 255) / 256;
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(k_fm_keep, dim3((unsigned)blocks, nchan), dim3(256), 0, s, a);
}

}  // namespace fm
}  // namespace nrsc5
