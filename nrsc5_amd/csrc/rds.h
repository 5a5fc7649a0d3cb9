// RDS / RBDS of the analog host (include/nrsc5hip.h, "RDS"): what the host unit (rds.hip), the kernels (k_rds.hip) and the analog
// FM object (fm_audio.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nrsc5hip.h"

struct nrsc5hip_fm;

namespace nrsc5 {
namespace rds {

constexpr int DEN = 11907, SC_NUM = 1824;      // 57 kHz = 1824 / 11907 cycles per Fs1 sample
constexpr int S = 8, GRID = 304;               // grid point r at 11907 r / 304 samples: 8 per bit
constexpr int HALF = 627, NT = 2 * HALF + 1;   // taps j = -HALF .. HALF around floor(t_r): every |m - t_r| <= 2 T is among them
constexpr int MT = 64;                         // grid points of one k_rds_mf tile
constexpr int MF_SPAN = 3728;                  // >= floor(11907 (r + 63) / 304) - floor(11907 r / 304) + NT = 2468 + 1255, float2 in LDS
constexpr int WIN_BITS = 152, WIN_PTS = WIN_BITS * S;
constexpr int WIN_MAX_BITS = WIN_BITS + 1, BITS_STRIDE = 160;
constexpr int NSTATS = NRSC5HIP_RDS_NSTATS;
constexpr int ST_BITS = 0, ST_VALID = 1, ST_CORRECTED = 2, ST_INVALID = 3, ST_GROUPS = 4, ST_DROPPED = 5, ST_GAINED = 6, ST_LOST = 7, ST_SEAM_DROPS = 8,
              ST_SEAM_INSERTS = 9, ST_TYPE0 = 10, ST_EVENTS = 42;
constexpr int LOSS_BLOCKS = 16;
constexpr unsigned EVENT_MAX = 64 + 64;        // header and the longest text
constexpr unsigned EVENTS_PER_GROUP = 6;       // raw group, PI twice (A and C'), and one of PS / RadioText / clock: 4, and room to spare

struct Event {                                 // as it lies in a channel's arena, followed by len bytes padded to 4
    uint32_t pos, len;                         // channel, bytes of text
    uint16_t kind, pad;
    uint32_t pad2;
    long long group, bit;                      // absolute group index since the last reset, index of the bit that completed the group
    int32_t v[8];
};
static_assert(sizeof(Event) == 64, "event header");

struct State {                                 // one channel's decoder between launches (all 32-bit words: copied to LDS and back as such)
    long long nbits, ngroups, gindex;
    unsigned reg;
    int synced, exp, fill, bad_run, in_group, gmask;
    int gw[4];
    int ring[26];                              // class << 8 | run length of the word that ended at this position mod 26; class 255: none
    int pi, pty, tp, ta, ms, di;
    int ps_mask, ps_have;
    int rt_mask, rt_ab, rt_ver, rt_have, rt_last_len;
    int clk_have, clk[4];
    unsigned char ps_buf[8], ps_last[8], rt_buf[64], rt_last[64];
};
static_assert(sizeof(State) % 8 == 0, "State is moved as words");

inline void state_init(State &s)
{
    s = State();
    for (int &r : s.ring) r = 255 << 8;
    s.pi = -1; s.rt_ab = -1; s.rt_ver = -1; s.rt_last_len = -1;
}

struct MfArgs {
    const float *d; long long d_stride, d_base;          // d[m] of channel c at d[c * d_stride + m - d_base]
    const float2 *cs;                                    // [DEN] (cos, sin) of 2 pi k / DEN
    const float *tab;                                    // [NT][GRID]: tap j of grid point r at tab[j * GRID + r % GRID]
    float2 *y; long long y_stride, y_base;               // y[r] of channel c at y[c * y_stride + r - y_base]
    long long r0, r_count;                               // the new grid points [r0, r0 + r_count)
};

struct BitsArgs {
    const float2 *y; long long y_stride, y_base;
    long long w0; int nwin;                              // windows [w0, w0 + nwin)
    const int *s_in; int *s_out;                         // [nchan]: s of window w0 - 1 (-1: none), s of the last window
    uint8_t *bits; int *counts;                          // [nchan][nwin][BITS_STRIDE], [nchan][nwin]
    float *energy; int *s_w;                             // optional (stage hook): [nchan][nwin][S], [nchan][nwin]
    unsigned long long *stats;                           // optional: [nchan][NSTATS], the seam counters
};

struct GroupsArgs {
    const int *targets;                                  // optional: the channel of workgroup i
    const uint8_t *bits; long long chan_stride, seg_stride;   // segment g of workgroup i at bits + i * chan_stride + g * seg_stride
    const int *counts; int nseg;                         // [workgroups][nseg]
    const int *reset_at;                                 // optional [workgroups]: the state is reset in front of this bit of the call (-1: never)
    State *state; unsigned long long *stats;
    uint8_t *arena; unsigned *used; unsigned *overflow; unsigned arena_cap;   // channel c's events at arena + c * arena_cap, used[c] bytes of them
    int raw, burst;
};

struct KeepArgs { const float2 *y_old; float2 *y_new; long long y_stride, shift, count; };

void launch_mf(hipStream_t s, int tiles, int nchan, const MfArgs &a);
void launch_bits(hipStream_t s, int nchan, const BitsArgs &a);
void launch_groups(hipStream_t s, int nwg, const GroupsArgs &a);
void launch_keep(hipStream_t s, int nchan, const KeepArgs &a);

// grid points whose last tap lies inside m_total samples of d
inline long long points_total(long long m_total) { return m_total < HALF + 1 ? 0 : ((long long)GRID * (m_total - HALF - 1) + GRID - 1) / DEN + 1; }

}  // namespace rds

struct RdsHost;
// the RDS half of fm_launch: matched filter, decisions and groups of what the front end has just added to d (d holds [d_base, m1)), on `s`; no host
// wait but where a buffer has to grow (y, one launch's decisions) or the bound of the unread events has filled the arenas: then the stream is waited
// for and the bytes really used are read back (4 per channel) before anything grows
int rds_launch(nrsc5hip_fm *f, hipStream_t s, const float *d, long long m1);
long long rds_d_need(const nrsc5hip_fm *f);              // the first d[m] the next call reads
int rds_reset(nrsc5hip_fm *f);
void rds_free(RdsHost *r);
}  // namespace nrsc5
