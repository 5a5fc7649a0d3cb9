// Carrier quality of the analog host (include/nrsc5hip.h, "carrier quality"; the definition: DESIGN.md (q)): moments of the channel-filtered
// envelope r[m] = |z[m]|^2 (k_fm_front writes it next to d when the measurement is enabled) and the mean of the discriminator.
//
// Every quantity is a function of absolute sample indices and every sum has a stated order: any chunking gives the same bits.  No atomics.
//   k_fm_carrier         one wave = one complete block j of one channel: s2 = sum r, s4 = sum r^2, s1 = sum d over m in [540 j, 540 j + 540),
//                        in double; lane l takes m = 540 j + l + 64 i, i ascending, then an xor butterfly (k_fm_pilot's order).
//   k_fm_carrier_report  one wave = one channel, once per push that completed a block: the windowed triple of the last audio block delivered
//                        (33 block triples under the pilot's window, a butterfly), the push's new blocks added to the running triple in block
//                        order (lane q < 3 adds component q, one block after the other), and the kept tails: the last 33 block triples and
//                        the r of the incomplete block move into the other buffer.
#include <hip/hip_runtime.h>
#include "fm_audio.h"

namespace nrsc5 {
namespace fm {
namespace {

__device__ __forceinline__ double wave_sum(double v)
{
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);  // a + b == b + a: every lane ends with the same bits
    return v;
}

__global__ __launch_bounds__(64) void k_fm_carrier(CarrierArgs a)
{
    const int ch = blockIdx.y;
    const long long j = a.j0 + blockIdx.x;
    const float *r = a.r + (long long)ch * a.r_stride + ((long long)BLOCK * j - a.r_base);
    const float *d = a.d + (long long)ch * a.d_stride + ((long long)BLOCK * j - a.d_base);
    double s2 = 0.0, s4 = 0.0, s1 = 0.0;
    for (int mi = threadIdx.x; mi < BLOCK; mi += 64) {
        const double v = (double)r[mi];
        s2 += v; s4 += v * v;                                // the product of two float32 values is exact in double
        s1 += (double)d[mi];
    }
    s2 = wave_sum(s2); s4 = wave_sum(s4); s1 = wave_sum(s1);
    if (threadIdx.x < 3) a.t[3 * ((long long)ch * a.t_stride + (j - a.t_base)) + threadIdx.x] = threadIdx.x == 0 ? s2 : threadIdx.x == 1 ? s4 : s1;
}

__global__ __launch_bounds__(64) void k_fm_carrier_report(ReportArgs a)
{
    const int ch = blockIdx.x, lane = threadIdx.x;
    const double *t = a.t + 3 * (long long)ch * a.t_stride;
    double *rep = a.report + 6 * ch;
    if (a.ja >= 0) {                                         // blocks ja - W .. ja + W, the ones in front of the stream zero
        double w2 = 0.0, w4 = 0.0, w1 = 0.0;
        const long long jb = a.ja + lane - W;
        if (lane <= 2 * W && jb >= 0) {
            const double *v = t + 3 * (jb - a.t_base);
            const double w = (double)a.win[lane];
            w2 = v[0] * w; w4 = v[1] * w; w1 = v[2] * w;
        }
        w2 = wave_sum(w2); w4 = wave_sum(w4); w1 = wave_sum(w1);
        if (lane < 3) rep[lane] = lane == 0 ? w2 : lane == 1 ? w4 : w1;
    }
    if (lane < 3) {
        double s = rep[3 + lane];
        for (long long j = a.j0; j < a.j1; j++) s += t[3 * (j - a.t_base) + lane];
        rep[3 + lane] = s;
    }
    const long long nt = 3 * (a.j1 - a.t_base_new), shift = 3 * (a.t_base_new - a.t_base);
    double *tn = a.t_new + 3 * (long long)ch * a.t_stride;
    for (long long i = lane; i < nt; i += 64) tn[i] = t[i + shift];
    const float *ro = a.r_old + (long long)ch * a.r_stride + a.r_shift;
    float *rn = a.r_new + (long long)ch * a.r_stride;
    for (long long i = lane; i < a.r_count; i += 64) rn[i] = ro[i];
}

}  // namespace

void launch_carrier(hipStream_t s, int blocks, int nchan, const CarrierArgs &a)
{
    count_launch();
    hipLaunchKernelGGL(k_fm_carrier, dim3(blocks, nchan), dim3(64), 0, s, a);
}

void launch_carrier_report(hipStream_t s, int nchan, const ReportArgs &a)
{
    count_launch();
    hipLaunchKernelGGL(k_fm_carrier_report, dim3(nchan), dim3(64), 0, s, a);
}

}  // namespace fm
}  // namespace nrsc5
