// Reception impairments of the analog host (include/nrsc5hip.h, "reception impairments"): what the host unit (fm_impair.hip), the
// kernels (k_fm_impair.hip) and the analog FM object (fm_audio.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nrsc5hip.h"

struct nrsc5hip_fm;

namespace nrsc5 {
namespace fm {

constexpr int UT = NRSC5HIP_FM_IMPAIR_TAPS;       // taps of hU
constexpr int NS = NRSC5HIP_FM_IMPAIR_NSUMS;      // sums per block record
constexpr int R_TAIL = UT + 1;                    // e[540 j - (UT - 1)] reads r[540 j - UT]: the r kept in front of the first incomplete block
constexpr int RECORDS_KEPT = 33;                  // 2 W + 1: the block records the windowed report of the next audio block reads

struct ImpairArgs {
    const float *r; long long r_stride, r_base;      // r[m], m >= r_base, of channel c at r[c * r_stride + m - r_base]
    const float *r_tail;                             // r[r_base - R_TAIL, r_base) of channel c at r_tail[c * R_TAIL ..]; not read when r_base == 0
    const float *d; long long d_stride, d_base;      // d[m] of channel c at d[c * d_stride + m - d_base]; d_base <= max(0, 540 j0 - UT)
    const float *hu;                                 // [UT]
    double *t; long long t_stride, t_base;           // the record of block j of channel c at t[NS * (c * t_stride + j - t_base)]
    long long j0;                                    // blocks [j0, j0 + gridDim.x)
    float *e_out, *eu_out, *du_out; long long out_stride;    // stage hook: sample m of channel c at [c * out_stride + m]; nullptr: not written
};

struct ImpairReportArgs {
    const double *t; double *t_new; long long t_stride, t_base, t_base_new;     // t_new holds the records [t_base_new, j1)
    long long j0, j1;                                // the push's new blocks
    long long ja;                                    // the last audio block delivered, -1: none yet
    const float *win;                                // [2 W + 1]
    double *report;                                  // [nchan][2 NS]: the windowed sums, the running sums
    const float *r; long long r_stride, r_at;        // the new tail: r_tail[c * R_TAIL + i] = r[c * r_stride + r_at + i], i < R_TAIL
    float *r_tail;
};

void launch_impair(hipStream_t s, int blocks, int nchan, const ImpairArgs &a);
void launch_impair_report(hipStream_t s, int nchan, const ImpairReportArgs &a);

}  // namespace fm

struct ImpairHost;
// room for the records up to b1: grown once the work queued on `s` has finished; what is kept moves over
int impair_reserve(nrsc5hip_fm *f, hipStream_t s, long long b1);
// the block records of the new blocks [f->blocks, b1), then the reports and the kept tails: two launches, called behind carrier_launch_sums and in
// front of carrier_launch_report (which hands r over to the other buffer), while f still holds the counts in front of the push
int impair_launch(nrsc5hip_fm *f, hipStream_t s, const float *d, long long b1, long long a1);
int impair_reset(nrsc5hip_fm *f);
void impair_free(ImpairHost *p);
}  // namespace nrsc5
