// Carrier quality of the analog host (include/nrsc5hip.h, "carrier quality"): what the host unit (fm_carrier.hip), the kernels
// (k_fm_carrier.hip) and the analog FM object (fm_audio.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nrsc5hip.h"

struct nrsc5hip_fm;

namespace nrsc5 {
namespace fm {

// 2 W + 1: the block triples the windowed report of the next audio block reads.  The steered audio kernel reads one audio block further back, the
// window of block a1 - 1 in front of the push's first new block a1, that is from block a1 - 1 - W = b1 - 2 W - 1 of the push before: the oldest kept
constexpr int TRIPLES_KEPT = 33;

struct CarrierArgs {
    const float *r; long long r_stride, r_base;      // r[m] of channel c at r[c * r_stride + m - r_base]
    const float *d; long long d_stride, d_base;
    double *t; long long t_stride, t_base;           // {s2, s4, s1} of block j of channel c at t[3 * (c * t_stride + j - t_base)]
    long long j0;                                    // blocks [j0, j0 + gridDim.x)
};

struct ReportArgs {
    const double *t; double *t_new; long long t_stride, t_base, t_base_new;     // t_new holds the triples [t_base_new, j1)
    long long j0, j1;                                // the push's new blocks
    long long ja;                                    // the last audio block delivered, -1: none yet
    const float *win;                                // [2 W + 1]
    double *report;                                  // [nchan][6]: the windowed triple, the running triple
    const float *r_old; float *r_new; long long r_stride, r_shift, r_count;     // r_new[i] = r_old[i + r_shift], i < r_count: the incomplete block
};

void launch_carrier(hipStream_t s, int blocks, int nchan, const CarrierArgs &a);
void launch_carrier_report(hipStream_t s, int nchan, const ReportArgs &a);

}  // namespace fm

struct CarrierHost;
struct FrontTarget { float *r; long long r_stride, r_base; };
// room for r[540 blocks, m1) and the triples up to b1: grown once the work queued on `s` has finished; what is kept moves over
int carrier_reserve(nrsc5hip_fm *f, hipStream_t s, long long m1, long long b1);
FrontTarget carrier_front(const nrsc5hip_fm *f);         // where k_fm_front writes r in this push
// the block sums of the new blocks [f->blocks, b1), then the reports and the kept tails: two launches, called in this order while f still holds
// the counts in front of the push.  Unsteered both follow the audio; a steered object runs the sums in front of it, and its audio
// kernel reads the triples where carrier_triples says
int carrier_launch_sums(nrsc5hip_fm *f, hipStream_t s, const float *d, long long b1);
int carrier_launch_report(nrsc5hip_fm *f, hipStream_t s, long long m1, long long b1, long long a1);
struct Triples { const double *t; long long t_stride, t_base; };
Triples carrier_triples(const nrsc5hip_fm *f);           // in this push, in front of carrier_launch_report
int carrier_enable(nrsc5hip_fm *f);                      // nrsc5hip_fm_carrier_enable behind its checks
int carrier_reset(nrsc5hip_fm *f);
void carrier_free(CarrierHost *c);
}  // namespace nrsc5
