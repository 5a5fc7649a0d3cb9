// EAS alerts (SAME) of the analog host (include/nrsc5hip.h, "SAME"): what the host unit (same.hip), the kernels (k_same.hip) and
// the analog FM object (fm_audio.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nrsc5hip.h"

struct nrsc5hip_fm;

namespace nrsc5 {
namespace same {

constexpr int DEN = 35721, K_MARK = 200, K_SPACE = 150;   // mark 6250/3 Hz = 200 / 35721, space 1562.5 Hz = 150 / 35721 cycles per Fs1 sample
constexpr int S = 8, GRID = 400;               // grid point r starts at floor(35721 r / 400) samples: 8 per bit, a bit is 35721 / 50 samples
constexpr int TT = 64;                         // segments of one k_same_tones tile
constexpr int TONE_SPAN = 5717;                // >= floor(35721 (r + 64) / 400) - floor(35721 r / 400) = 5715 or 5716, floats in LDS
constexpr int WIN_BITS = 64, WIN_PTS = WIN_BITS * S;
constexpr int WIN_MAX_BITS = WIN_BITS + 1, BITS_STRIDE = 72;
constexpr int TAIL = S - 1;                    // q[r] reads c[r .. r + 7]: a window is decided once c[512 (w + 1) + 6] exists
constexpr int TEXT_MAX = NRSC5HIP_SAME_TEXT_MAX, TEXT_PAD = 272;
constexpr int VOTE_BITS = 2604;                // 5 s
constexpr int NSTATS = NRSC5HIP_SAME_NSTATS;
constexpr int ST_BITS = 0, ST_PREAMBLES = 1, ST_BURSTS = 2, ST_ABORTED = 3, ST_MESSAGES = 4, ST_NO_MESSAGE = 5, ST_EOM = 6, ST_SEAM_DROPS = 7,
              ST_SEAM_INSERTS = 8, ST_EVENTS = 9;
constexpr int SEARCH = 0, PREAMBLE = 1, MESSAGE = 2;
constexpr int KIND_HEADER = 1, KIND_EOM = 2;
constexpr unsigned EVENT_MAX = 64 + TEXT_PAD;  // header and the longest text
constexpr unsigned BURST_MIN_BITS = 48;        // 16 bits of preamble and NNNN: no burst is shorter, and a burst yields at most two events

struct Event {                                 // as it lies in a channel's arena, followed by len bytes padded to 4
    uint32_t pos, len;                         // channel, bytes of text
    uint16_t kind, pad;
    uint32_t pad2;
    long long first, last;                     // bit index (since the last reset) of the first bit of the text and of its last bit
    int32_t v[8];
};
static_assert(sizeof(Event) == 64, "event header");

struct State {                                 // one channel's framer and vote between launches (moved to LDS and back as 32-bit words)
    long long nbits;
    long long pre_bit, first_bit;              // the preamble match and the first bit of the message being read
    long long grp_last;                        // last bit of the newest burst of the group
    long long msg_first, msg_last;             // of the last message: first bit of the burst that decided it, last bit of that burst
    unsigned reg;                              // the last 16 bits, the newest in bit 15
    int state, fill, len;
    int grp_kind, grp_n, grp_done;             // bursts of the current group; done: 1 a message was produced, 2 the three never agreed (counted)
    int grp_len[3];
    int msg_len, msg_kind, pad[2];              // the last message (msg_len -1: none)
    unsigned char buf[TEXT_PAD], grp[3][TEXT_PAD], msg[TEXT_PAD];
};
static_assert(sizeof(State) % 8 == 0, "State is moved as words");

inline void state_init(State &s)
{
    s = State();
    s.msg_len = -1;
}

struct TonesArgs {
    const float *d; long long d_stride, d_base;          // d[m] of channel c at d[c * d_stride + m - d_base]
    const float2 *cs;                                    // [DEN] (cos, sin) of 2 pi k / DEN
    float4 *c; long long c_stride, c_base;               // (Re c_1, Im c_1, Re c_0, Im c_0)[r] of channel c at c[c * c_stride + r - c_base]
    long long r0, r_count;                               // the new segments [r0, r0 + r_count)
};

struct BitsArgs {
    const float4 *c; long long c_stride, c_base;
    long long w0; int nwin;                              // windows [w0, w0 + nwin)
    const int *s_in; int *s_out;                         // [nchan]: s of window w0 - 1 (-1: none), s of the last window
    uint8_t *bits; int *counts;                          // [nchan][nwin][BITS_STRIDE], [nchan][nwin]
    float *q, *metric; int *s_w;                         // optional (stage hook): [nchan][nwin][WIN_PTS], [nchan][nwin][S], [nchan][nwin]
    unsigned long long *stats;                           // optional: [nchan][NSTATS], the seam counters
};

struct FramesArgs {
    const int *targets;                                  // optional: the channel of workgroup i
    const uint8_t *bits; long long chan_stride, seg_stride;   // segment g of workgroup i at bits + i * chan_stride + g * seg_stride
    const int *counts; int nseg;                         // [workgroups][nseg]
    const int *reset_at;                                 // optional [workgroups]: the state is reset in front of this bit of the call (-1: never)
    State *state; unsigned long long *stats;
    uint8_t *arena; unsigned *used; unsigned *overflow; unsigned arena_cap;   // channel c's events at arena + c * arena_cap, used[c] bytes of them
    int burst_events;                                    // also a BURST event per burst
};

struct KeepArgs { const float4 *c_old; float4 *c_new; long long c_stride, shift, count; };

void launch_tones(hipStream_t s, int tiles, int nchan, const TonesArgs &a);
void launch_bits(hipStream_t s, int nchan, const BitsArgs &a);
void launch_frames(hipStream_t s, int nwg, const FramesArgs &a);
void launch_keep(hipStream_t s, int nchan, const KeepArgs &a);

constexpr long long grid_floor(long long r) { return ((long long)DEN * r) / GRID; }
// segments that lie inside m_total samples of d: the r with floor(35721 (r + 1) / 400) <= m_total
inline long long segments_total(long long m_total) { return m_total < 0 ? 0 : ((long long)GRID * (m_total + 1) - 1) / DEN; }
inline long long windows_total(long long segs) { return segs < TAIL ? 0 : (segs - TAIL) / WIN_PTS; }

}  // namespace same

struct SameHost;
// the SAME half of fm_launch: tone sums, decisions and framing of what the front end has just added to d (d holds [d_base, m1)), on `s`; no host
// wait but where a buffer has to grow (c, one launch's decisions) or the bound of the unread events has filled the arenas
int same_launch(nrsc5hip_fm *f, hipStream_t s, const float *d, long long m1);
long long same_d_need(const nrsc5hip_fm *f);             // the first d[m] the next call reads
int same_reset(nrsc5hip_fm *f);
void same_free(SameHost *r);
}  // namespace nrsc5
