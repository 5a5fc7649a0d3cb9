// Analog FM audio (include/nrsc5hip.h, "analog FM audio"): what the host units (through fm_host.h, which holds the object itself),
// the kernels (k_fm_audio.hip) and the channelizer's feed (k_channelize.hip) share: constants, the kernels' arguments and their launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "nrsc5hip.h"
#include "rds.h"
#include "same.h"
#include "fm_carrier.h"
#include "fm_impair.h"

namespace nrsc5 {
namespace fm {

constexpr int TA = 112;                       // channel filter taps
constexpr int HIST = TA + 2;                  // input samples kept per channel: z[m - 1] of the first new m reads back to 2 (m - 1) - (TA - 1)
constexpr int FT = 256;                       // Fs1 outputs of one k_fm_front tile
constexpr int PHASES = 16, T_NUM = 135;       // audio output k at t_k = 135 k / 16 Fs1 samples
constexpr int BLOCK = 540, BLOCK_OUT = 64;    // one pilot block: 540 Fs1 samples = 64 audio outputs
constexpr int PILOT_NUM = 608, PILOT_DEN = 11907;   // 19 kHz = 608 / 11907 cycles per Fs1 sample
constexpr float DEV_SCALE = (float)(372093.75 / (2.0 * 3.14159265358979323846 * 75000.0));   // Fs1 / (2 pi 75 kHz): +-75 kHz -> +-1
constexpr int W = 16;                         // pilot smoothing over 2 W + 1 blocks

// reception steering: the three ramps in q as the device applies them, f = min(1, max(0, ((float)q - lo) * inv)); a control that is off has factor 1
struct SteerRamps {
    unsigned controls;                        // NRSC5HIP_FM_STEER_*
    float blend_lo, blend_inv, highcut_lo, highcut_inv, mute_lo, mute_inv, mute_floor;
};

struct FrontArgs {
    const int16_t *in; long long in_stride;   // channel c's new input at in + c * in_stride: absolute samples [n0, n0 + n_in)
    long long n0, n_in;
    const int *hist;                          // [nchan][HIST] cs16 pairs: absolute samples [n0 - HIST, n0), zero before n = 0
    const float *ha;                          // [TA]
    float *d; long long d_stride, d_base;     // d[m] of channel c at d[c * d_stride + m - d_base]
    long long m0, m_count;                    // the new outputs [m0, m0 + m_count)
    float *r = nullptr; long long r_stride = 0, r_base = 0;   // carrier measurement: r[m] of channel c at r[c * r_stride + m - r_base]; nullptr: not written
};

struct PilotArgs {
    const float *d; long long d_stride, d_base;
    const float2 *cs;                         // [PILOT_DEN] (cos, sin) of 2 pi k / PILOT_DEN
    float2 *p; long long p_stride, p_base;    // block sum j of channel c at p[c * p_stride + j - p_base]
    long long j0;                             // blocks [j0, j0 + gridDim.x)
};

struct AudioArgs {
    const float *d; long long d_stride, d_base;
    const float2 *p; long long p_stride, p_base;
    const float2 *cs;
    const float *tab; int tb;                 // [tb][PHASES]: tab[j * 16 + p] = g[16 j + p]
    const float *win; float wsum;             // [2 W + 1]
    float aq, bq, pilot_min;
    const float *scale;                       // [nchan] 32767 * gain
    long long j0, k0;                         // audio blocks [j0, j0 + gridDim.x); output k goes to out[.. + 2 (k - k0)]
    int16_t *out; long long out_stride;
    unsigned long long *clips;                // [nchan][2]
    float *pilot;                             // [nchan][2]: level and stereo flag of the last block
};

// reception steering (k_fm_audio<true>): what the steered kernel reads on top.  A struct of its own: the unsteered kernel's arguments
// stay as they were, to the byte
struct SteeredAudioArgs : AudioArgs {
    const double *t; long long t_stride, t_base;             // k_fm_carrier's block triples: block j of channel c at t[3 * (c * t_stride + j - t_base)]
    const float *tab_n;                       // [tb][PHASES]: the narrow table, laid out as tab
    SteerRamps ramps;
    float4 *steer; long long steer_stride;    // (q, b, h, g) of channel c's last block at steer[c * steer_stride] ...
    int steer_every;                          // ... or, for the stage hook, of every block: block j0 + i at steer[c * steer_stride + i]
};

struct KeepArgs {
    const float *d_old; float *d_new; long long d_stride, d_shift, d_count;     // d_new[i] = d_old[i + d_shift], i < d_count
    const float2 *p_old; float2 *p_new; long long p_stride, p_shift, p_count;
    const int16_t *in; long long in_stride, n0, n_in;
    const int *hist_old; int *hist_new;
};

// Where the launch_* functions of k_fm_audio.hip, k_fm_carrier.hip, k_fm_impair.hip, k_rds.hip and k_same.hip count themselves, one per kernel launch: fm_launch points it at its object's counter
// for the length of a push (nrsc5hip_fm_debug_launches); nullptr anywhere else (the stage hooks are not counted)
extern thread_local long long *launch_count;
inline void count_launch() { if (launch_count) ++*launch_count; }
struct CountLaunches {
    explicit CountLaunches(long long *to) { launch_count = to; }
    ~CountLaunches() { launch_count = nullptr; }
};

double bessel_i0(double x);                   // the filter designs' Kaiser window, in double (fm_audio.hip)

void launch_front(hipStream_t s, int tiles, int nchan, const FrontArgs &a);
void launch_pilot(hipStream_t s, int blocks, int nchan, const PilotArgs &a);
void launch_audio(hipStream_t s, int blocks, int nchan, const AudioArgs &a);
void launch_audio_steered(hipStream_t s, int blocks, int nchan, const SteeredAudioArgs &a);
void launch_keep(hipStream_t s, int nchan, const KeepArgs &a);

}  // namespace fm
}  // namespace nrsc5

namespace nrsc5 {
// for nrsc5hip_chan_feed_fm: the checks of nrsc5hip_fm_process without its launch, and the launch without a wait, on the caller's stream
int fm_nchan(const nrsc5hip_fm *fm);
int fm_device(const nrsc5hip_fm *fm);
int fm_check(nrsc5hip_fm *fm, long long n_in, const int16_t *dev_out, long long out_stride_elems, long long out_capacity, long long *n_out);
int fm_launch(nrsc5hip_fm *fm, hipStream_t stream, const int16_t *dev_in, long long in_stride_elems, long long n_in, int16_t *dev_out,
              long long out_stride_elems);
}  // namespace nrsc5
