// Reception impairments of the analog host (include/nrsc5hip.h, "reception impairments"; the definition: DESIGN.md (t)): the amplitude
// e[m] = sqrt(r[m] r[m - 1]) against the discriminator d[m] -- moments for a quadratic fit of e on d (multipath), and the correlation of the two
// behind a 100 .. 170 kHz band-pass (a neighbour on one side).
//
// Every quantity is a function of absolute sample indices and every sum has a stated order: any chunking gives the same bits.  No atomics.
//   k_fm_impair         one wave = one complete block j of one channel.  e and d of [540 j - 62, 540 j + 540) go to LDS (e from r, whose 64
//                       samples in front of the first new block come from the kept tail), the two 63-tap FIRs run from LDS with the tap uniform
//                       across the wave (lane l holds the outputs m = 540 j + l + 64 i in registers, the tap loop outside: one float32 fma chain
//                       per output, taps ascending), then the eleven sums in double in k_fm_carrier's order and one record per block.
//   k_fm_impair_report  one wave = one channel, once per push that completed a block: the windowed sums of the last audio block delivered (33
//                       block records under the pilot's window, a butterfly per sum), the push's new blocks added to the running sums in block
//                       order (lane q < 11 adds sum q), and the kept tails: the last 33 records move into the other buffer, the last 64 r in
//                       front of the incomplete block into the tail.
#include <hip/hip_runtime.h>
#include "fm_audio.h"
#include "fm_impair.h"

namespace nrsc5 {
namespace fm {
namespace {

constexpr int HALO = UT - 1;                       // samples in front of the block that its first output reads
constexpr int NI = (BLOCK + 63) / 64;              // outputs per lane; the last one only in lanes l + 64 (NI - 1) < 540
constexpr int STAGED = HALO + 64 * NI;             // the lanes without a last output read up to here: zero behind the block

__device__ __forceinline__ double wave_sum(double v)
{
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);  // a + b == b + a: every lane ends with the same bits
    return v;
}

static_assert(R_TAIL == 64, "k_fm_impair_report moves the tail with one lane per sample");

// r[m], m >= 0: from this push's r, or from the tail kept in front of it
__device__ __forceinline__ float r_at(const float *r, const float *tail, long long r_base, long long m)
{
    return m >= r_base ? r[m - r_base] : tail[m - (r_base - R_TAIL)];
}

__global__ __launch_bounds__(64) void k_fm_impair(ImpairArgs a)
{
    __shared__ float e_s[STAGED], d_s[STAGED];
    const int ch = blockIdx.y, lane = threadIdx.x;
    const long long j = a.j0 + blockIdx.x, m_first = (long long)BLOCK * j - HALO;
    const float *r = a.r + (long long)ch * a.r_stride;
    const float *tail = a.r_tail + (long long)ch * R_TAIL;
    const float *d = a.d + (long long)ch * a.d_stride;
    for (int idx = lane; idx < STAGED; idx += 64) {
        const long long m = m_first + idx;
        float e = 0.0f, x = 0.0f;
        // e[0] = 0 (there is no r[-1]) and d[0] = 0 (no z[-1]: k_fm_front writes 0 there), by definition; in front of the stream both are zero
        if (idx < HALO + BLOCK && m >= 1) {
            const float r1 = r_at(r, tail, a.r_base, m), r0 = r_at(r, tail, a.r_base, m - 1);
            e = sqrtf(r1 * r0);
            x = d[m - a.d_base];
        }
        e_s[idx] = e; d_s[idx] = x;
        if (a.e_out && idx >= HALO && idx < HALO + BLOCK) a.e_out[(long long)ch * a.out_stride + m] = e;
    }
    __syncthreads();
    float eu[NI], du[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) eu[i] = du[i] = 0.0f;
    for (int t = 0; t < UT; t++) {
        const float h = a.hu[t];
        const int at = HALO + lane - t;
#pragma unroll
        for (int i = 0; i < NI; i++) {
            eu[i] = fmaf(h, e_s[at + 64 * i], eu[i]);
            du[i] = fmaf(h, d_s[at + 64 * i], du[i]);
        }
    }
    double s[NS];
#pragma unroll
    for (int q = 0; q < NS; q++) s[q] = 0.0;
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int mi = lane + 64 * i;
        if (mi < BLOCK) {
            const double x = (double)d_s[HALO + mi], y = (double)e_s[HALO + mi], x2 = x * x, u = (double)eu[i], v = (double)du[i];
            s[0] += x; s[1] += x2; s[2] += x2 * x; s[3] += x2 * x2;
            s[4] += y; s[5] += x * y; s[6] += x2 * y; s[7] += y * y;
            s[8] += u * u; s[9] += v * v; s[10] += u * v;
            if (a.eu_out) a.eu_out[(long long)ch * a.out_stride + (long long)BLOCK * j + mi] = eu[i];
            if (a.du_out) a.du_out[(long long)ch * a.out_stride + (long long)BLOCK * j + mi] = du[i];
        }
    }
    double mine = 0.0;
#pragma unroll
    for (int q = 0; q < NS; q++) {
        const double v = wave_sum(s[q]);
        mine = lane == q ? v : mine;
    }
    if (lane < NS) a.t[NS * ((long long)ch * a.t_stride + (j - a.t_base)) + lane] = mine;
}

__global__ __launch_bounds__(64) void k_fm_impair_report(ImpairReportArgs a)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    const double *t = a.t + NS * (long long)ch * a.t_stride;
    double *rep = a.report + 2 * NS * ch;
    if (a.ja >= 0) {                                         // blocks ja - W .. ja + W, the ones in front of the stream zero
        const long long jb = a.ja + lane - W;
        const bool in = lane <= 2 * W && jb >= 0;
        const double w = in ? (double)a.win[lane] : 0.0;
        const double *v = t + NS * ((in ? jb : a.ja) - a.t_base);
        double mine = 0.0;
#pragma unroll
        for (int q = 0; q < NS; q++) {
            const double sum = wave_sum(in ? v[q] * w : 0.0);
            mine = lane == q ? sum : mine;
        }
        if (lane < NS) rep[lane] = mine;
    }
    if (lane < NS) {
        double s = rep[NS + lane];
        for (long long j = a.j0; j < a.j1; j++) s += t[NS * (j - a.t_base) + lane];
        rep[NS + lane] = s;
    }
    const long long nt = NS * (a.j1 - a.t_base_new), shift = NS * (a.t_base_new - a.t_base);
    double *tn = a.t_new + NS * (long long)ch * a.t_stride;
    for (long long i = lane; i < nt; i += 64) tn[i] = t[i + shift];
    a.r_tail[(long long)ch * R_TAIL + lane] = a.r[(long long)ch * a.r_stride + a.r_at + lane];     // R_TAIL == 64 lanes
}

}  // namespace

void launch_impair(hipStream_t s, int blocks, int nchan, const ImpairArgs &a)
{
    count_launch();
    hipLaunchKernelGGL(k_fm_impair, dim3(blocks, nchan), dim3(64), 0, s, a);
}

void launch_impair_report(hipStream_t s, int nchan, const ImpairReportArgs &a)
{
    count_launch();
    hipLaunchKernelGGL(k_fm_impair_report, dim3(nchan), dim3(64), 0, s, a);
}

}  // namespace fm
}  // namespace nrsc5
