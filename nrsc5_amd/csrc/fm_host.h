// Host plumbing shared by the units of the analog FM object (fm_audio.hip, fm_carrier.hip, fm_impair.hip, rds.hip, same.hip):
// the ping-pong array that grows, the per-channel event arena, the object that holds them, the opening of the stage hooks and the small shared
// pieces.  Host code only: no k_*.hip file includes this.
#pragma once
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "host_util.h"
#include "arena_consumer.h"
#include "fm_audio.h"

namespace nrsc5 {

// the input checks of nrsc5hip_fm_process, nrsc5hip_chan_feed_fm's caller and every stage hook (fm_audio.hip)
int fm_check_input(const nrsc5hip_fm *f, const void *dev_in, long long in_stride_elems, long long n_in);

namespace fm {

// A double-buffered per-channel device array: item i of channel c at p[cur][width * (c * cap + i - base)].  A push writes the half `cur`, its
// keep kernel moves what the next push needs to the other half, and the owner flips `cur`; `cur` and `base` stay with the owner (one `cur` may
// serve several arrays)
template <typename T> struct PingPong {
    T *p[2] = {nullptr, nullptr}; long long cap = 0;         // cap: items per channel
    PingPong() = default;
    PingPong(const PingPong &) = delete;
    PingPong &operator=(const PingPong &) = delete;
    ~PingPong() { (void)hipFree(p[0]); (void)hipFree(p[1]); }

    // create / enable: both halves with room for `items` per channel
    hipError_t alloc(long long items, int nchan, int width = 1)
    {
        cap = items;
        for (int i = 0; i < 2; i++) {
            const hipError_t e = hipMalloc(&p[i], sizeof(T) * width * (size_t)cap * nchan);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }

    // room for `need` items per channel: grown once the work queued on `s` has finished; the `have` items the half `cur` holds move over
    int reserve(hipStream_t s, long long need, long long have, int nchan, int width, long long slack, int cur, const char *what)
    {
        if (need <= cap) return 0;
        HIPCHK(hipStreamSynchronize(s));
        const long long grown = need + need / 4 + slack;
        const size_t item = sizeof(T) * width;
        T *n[2] = {nullptr, nullptr};
        HIPCHK(hipMalloc(&n[0], item * (size_t)grown * nchan));
        if (hipMalloc(&n[1], item * (size_t)grown * nchan) != hipSuccess) { (void)hipFree(n[0]); FAIL(NRSC5HIP_ENOMEM, "out of device memory (%s, %lld per channel)", what, grown); }
        hipError_t e = have > 0 ? hipMemcpy2DAsync(n[cur], item * grown, p[cur], item * cap, item * have, nchan, hipMemcpyDeviceToDevice, s) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(n[0]); (void)hipFree(n[1]); FAIL(NRSC5HIP_EHIP, "moving %s to its grown buffer failed: %s", what, hipGetErrorString(e)); }
        (void)hipFree(p[0]); (void)hipFree(p[1]);
        p[0] = n[0]; p[1] = n[1]; cap = grown;
        return 0;
    }
};

// The events of every channel between two reads (RDS, SAME): channel c's at d_arena + c * arena_cap, d_used[c] bytes of them, written by the unit's
// framing kernel; d_used[nchan] is the kernel's overflow flag.  Event: the record header (pos = channel, len = bytes of text behind it)
struct EventArena {
    uint8_t *d_arena = nullptr; DevFixed<unsigned> d_used;   // [nchan][arena_cap]; d_used: [nchan] bytes used, then the overflow flag
    unsigned arena_cap = 0; size_t pending = 0;              // pending: what a channel's arena may hold at most since the last look
    EventArena() = default;
    EventArena(const EventArena &) = delete;
    EventArena &operator=(const EventArena &) = delete;
    ~EventArena() { (void)hipFree(d_arena); }

    hipError_t alloc(size_t cap, int nchan)
    {
        arena_cap = (unsigned)cap;
        const hipError_t e = hipMalloc(&d_used.p, sizeof(unsigned) * ((size_t)nchan + 1));
        return e != hipSuccess ? e : hipMalloc(&d_arena, (size_t)arena_cap * nchan);
    }

    // no event and no overflow, on `s`
    int reset(hipStream_t s, int nchan)
    {
        HIPCHK(hipMemsetAsync(d_used.p, 0, sizeof(unsigned) * (nchan + 1), s));
        pending = 0;
        return 0;
    }

    // room in every channel's arena for `more` bytes of events on top of what may be unread; no host wait while the bound fits, else the bytes
    // really used are read back (4 per channel) and what the arenas hold moves over when they have to grow
    int reserve(hipStream_t s, size_t more, int nchan, const char *what)
    {
        if (pending + more <= arena_cap) { pending += more; return 0; }
        HIPCHK(hipStreamSynchronize(s));
        std::vector<unsigned> used((size_t)nchan);
        HIPCHK(hipMemcpy(used.data(), d_used.p, sizeof(unsigned) * nchan, hipMemcpyDeviceToHost));
        const size_t top = *std::max_element(used.begin(), used.end());
        pending = top;
        if (pending + more > arena_cap) {
            const size_t cap = 2 * (pending + more);
            if (cap * (size_t)nchan > 0xfffffff0u) FAIL(NRSC5HIP_EOVERFLOW, "%s events of %d channels unread: %zu bytes per channel", what, nchan, cap);
            uint8_t *na = nullptr;
            if (hipMalloc(&na, cap * nchan) != hipSuccess) FAIL(NRSC5HIP_ENOMEM, "out of device memory (%s events, %zu per channel)", what, cap);
            hipError_t e = top > 0 ? hipMemcpy2DAsync(na, cap, d_arena, arena_cap, top, nchan, hipMemcpyDeviceToDevice, s) : hipSuccess;
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { (void)hipFree(na); FAIL(NRSC5HIP_EHIP, "moving the %s events to their grown arena failed: %s", what, hipGetErrorString(e)); }
            (void)hipFree(d_arena);
            d_arena = na; arena_cap = (unsigned)cap;
        }
        pending += more;
        return 0;
    }

    // nrsc5hip_fm_*_read: fetches the used parts, empties the arenas and hands every event to deliver(channel, event, its text), channel by channel.
    // valid(event): the unit's own test of a header; kernel: who writes the arena, for the texts.  -> events delivered, or < 0
    template <typename Event, typename Valid, typename Deliver>
    int read(hipStream_t s, int nchan, const char *what, const char *kernel, Valid valid, Deliver deliver)
    {
        const size_t K = (size_t)nchan;
        HIPCHK(hipStreamSynchronize(s));
        std::vector<unsigned> used(K + 1);
        HIPCHK(hipMemcpy(used.data(), d_used.p, sizeof(unsigned) * (K + 1), hipMemcpyDeviceToHost));
        if (used[K]) FAIL(NRSC5HIP_EOVERFLOW, "%s event arena of %u bytes per channel too small: events are lost", what, arena_cap);
        const size_t top = *std::max_element(used.begin(), used.begin() + K);
        if (top == 0) { pending = 0; return 0; }
        if (top > arena_cap) FAIL(NRSC5HIP_EHIP, "%s event arena is not what %s writes (%zu bytes used of %u)", what, kernel, top, arena_cap);
        std::vector<uint8_t> got(top * K);
        HIPCHK(hipMemcpy2DAsync(got.data(), top, d_arena, arena_cap, top, K, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemsetAsync(d_used.p, 0, sizeof(unsigned) * K, s));
        HIPCHK(hipStreamSynchronize(s));
        pending = 0;
        int delivered = 0;
        for (size_t c = 0; c < K; c++) {
            std::vector<std::vector<size_t>> per;
            size_t bad = 0;
            const uint8_t *base = got.data() + c * top;
            if (!arena_walk<Event>(base, used[c], K, [&](const Event &ev) { return ev.pos == c && valid(ev); }, per, &bad))
                FAIL(NRSC5HIP_EHIP, "%s event arena of channel %zu is not what %s writes (offset %zu)", what, c, kernel, bad);
            for (size_t at : per[c]) {
                Event ev;
                memcpy(&ev, base + at, sizeof(ev));
                deliver((int)c, ev, base + at + sizeof(Event));
                delivered++;
            }
        }
        return delivered;
    }
};

}  // namespace fm
}  // namespace nrsc5

struct nrsc5hip_fm {
    int device = 0, nchan = 0, tb = 0;
    double deemphasis_us = 75.0;
    float pilot_min = 0.03f, aq = 0, bq = 0, wsum = 0;
    std::vector<float> ha, tab, scale;                       // tab: host copy [PHASES][tb]
    hipStream_t stream = nullptr;
    float *d_ha = nullptr, *d_tab = nullptr, *d_win = nullptr, *d_scale = nullptr, *d_pilot = nullptr;
    float2 *d_cs = nullptr;
    int *d_hist[2] = {nullptr, nullptr};
    nrsc5::fm::PingPong<float> d; long long d_base = 0;      // d[m], m in [d_base, m_total), of channel c at d.p[cur][c * d.cap + m - d_base]
    nrsc5::fm::PingPong<float2> p; long long p_base = 0;     // block sums [p_base, blocks)
    int cur = 0;                                             // of d_hist, d and p
    unsigned long long *d_clips = nullptr;
    long long n_total = 0, m_total = 0, blocks = 0, audio_blocks = 0;        // input samples, d samples, complete pilot blocks, audio blocks delivered
    long long launches = 0;                                  // kernel launches of the pushes since create / reset
    bool processed = false;                                  // a push has been launched since create
    nrsc5::RdsHost *rds = nullptr;                           // RDS (rds.hip), once enabled
    nrsc5::SameHost *same = nullptr;                         // EAS alerts (same.hip), once enabled
    nrsc5::CarrierHost *carrier = nullptr;                   // carrier quality (fm_carrier.hip), once enabled
    nrsc5::ImpairHost *impair = nullptr;                     // reception impairments (fm_impair.hip), once enabled: needs carrier
    bool steer = false;                                      // reception steering, once enabled: needs carrier
    nrsc5::fm::SteerRamps ramps = {};
    std::vector<float> tab_n;                                // the narrow table, host copy [PHASES][tb]
    float *d_tab_n = nullptr;
    float4 *d_steer = nullptr;                               // [nchan]: (q, b, h, g) of the last audio block delivered
};

namespace nrsc5 {
namespace fm {

// nrsc5hip_fm_*_stats: the N device counters of one channel, once the work queued on the object's stream has finished
template <int N> int read_channel_stats(const nrsc5hip_fm *f, const unsigned long long *dev, int channel, long long *stats)
{
    if (!stats || channel < 0 || channel >= f->nchan) FAIL(NRSC5HIP_EINVAL, "bad channel %d", channel);
    HIPCHK(hipStreamSynchronize(f->stream));
    unsigned long long v[N];
    HIPCHK(hipMemcpy(v, dev + (size_t)channel * N, sizeof(v), hipMemcpyDeviceToHost));
    for (int k = 0; k < N; k++) stats[k] = (long long)v[k];
    return 0;
}

// The opening of a stage hook: the input taken as a whole session that starts at sample 0, through the front end alone on f->stream, into
// scratch that goes with this object.  Everything behind launch_front is the hook's own
struct StageFront {
    DevTmp d, r, hist;                                       // [nchan][m1] d, [nchan][m1] r (want_r), [nchan][HIST] zeros
    long long m1 = 0, b1 = 0;                                // Fs1 samples, complete pilot blocks
    const float *df() const { return (const float *)d.p; }
    const float *rf() const { return (const float *)r.p; }

    // min_blocks: a hook that has nothing to do on fewer complete blocks returns 0 early; then nothing is allocated or launched here either
    int open(const nrsc5hip_fm *f, const int16_t *dev_in, long long in_stride_elems, long long n_in, bool want_r, long long min_blocks = 0)
    {
        if (n_in <= 0) FAIL(NRSC5HIP_EINVAL, "bad input (n_in %lld)", n_in);
        const int rc = fm_check_input(f, dev_in, in_stride_elems, n_in);
        if (rc) return rc;
        m1 = (n_in + 1) >> 1; b1 = m1 / BLOCK;
        if ((m1 + FT - 1) / FT > 0x7fffffffLL) FAIL(NRSC5HIP_EINVAL, "input too large (%lld samples)", n_in);
        if (b1 < min_blocks) return 0;
        const size_t K = (size_t)f->nchan;
        HIPCHK(hipMalloc(&d.p, sizeof(float) * (size_t)m1 * K));
        if (want_r) HIPCHK(hipMalloc(&r.p, sizeof(float) * (size_t)m1 * K));
        HIPCHK(hipMalloc(&hist.p, sizeof(int) * HIST * K));
        HIPCHK(hipMemsetAsync(hist.p, 0, sizeof(int) * HIST * K, f->stream));
        FrontArgs a;
        a.in = dev_in; a.in_stride = in_stride_elems; a.n0 = 0; a.n_in = n_in; a.hist = (const int *)hist.p; a.ha = f->d_ha;
        a.d = (float *)d.p; a.d_stride = m1; a.d_base = 0; a.m0 = 0; a.m_count = m1;
        if (want_r) { a.r = (float *)r.p; a.r_stride = m1; a.r_base = 0; }
        launch_front(f->stream, (int)((m1 + FT - 1) / FT), f->nchan, a);
        HIPCHK(hipGetLastError());
        return 0;
    }
};

// the Hann window over the 2 W + 1 blocks -W .. W: in double, and the table as the device reads it
inline double hann(int w) { return 0.5 * (1 + cos(M_PI * w / (W + 1))); }
inline std::vector<float> hann_window()
{
    std::vector<float> win(2 * W + 1);
    for (int w = -W; w <= W; w++) win[w + W] = (float)hann(w);
    return win;
}

inline double sinc(double x) { return x == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x); }

// a figure in dB inside NRSC5HIP_FM_CARRIER_DB_MIN .. _MAX; not a number: the lower end
inline double clamp_db(double v)
{
    const double lo = NRSC5HIP_FM_CARRIER_DB_MIN, hi = NRSC5HIP_FM_CARRIER_DB_MAX;
    return !(v >= lo) ? lo : v > hi ? hi : v;
}

}  // namespace fm
}  // namespace nrsc5

// the opening of an nrsc5hip_fm_*_enable: `what` is enabled once, and only before the first push
#define FM_ENABLE_CHECK(f, enabled, what)                                                                  \
    if (!(f)) FAIL(NRSC5HIP_EINVAL, "null demodulator");                                                   \
    if (enabled) FAIL(NRSC5HIP_EINVAL, "%s is enabled already", what);                                     \
    if ((f)->processed) FAIL(NRSC5HIP_EINVAL, "%s can be enabled only before the first push", what)
// the opening of a call that needs the unit f->host (named `what` in the text): from here on the object's device is current
#define FM_FEATURE_ENTER(f, host, what)                                                                    \
    if (!(f)) FAIL(NRSC5HIP_EINVAL, "null demodulator");                                                   \
    if (!(f)->host) FAIL(NRSC5HIP_EINVAL, "%s is not enabled on this object", what);                       \
    nrsc5::DeviceGuard guard((f)->device)
