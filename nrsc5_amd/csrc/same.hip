// EAS alerts (SAME) of the analog host, host side (include/nrsc5hip.h, "SAME"): the phasor table in double, the buffers an analog
// FM object gains with nrsc5hip_fm_same_enable, the launches fm_launch chains behind its front end, the event read-back and the two stage hooks.
// The kernels are in k_same.hip; c's buffer that grows, the event arena and the hooks' opening are fm_host.h's.
//   per push, host -> device: nothing (the launches carry their arguments)
//   per read, device -> host: 4 bytes per channel (the used part of its arena) and the used parts themselves (64 bytes + the text per event)
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>
#include "nrsc5hip.h"
#include "host_util.h"
#include "fm_host.h"

using namespace nrsc5;
using namespace nrsc5::same;

struct nrsc5::SameHost {
    int burst_events = 1;
    std::vector<float2> cs;                                  // host copy of the table
    DevFixed<float2> d_cs;                                   // [DEN] (cos, sin) of 2 pi k / DEN
    fm::PingPong<float4> c; long long c_base = 0; int cur = 0;   // c[r], r in [c_base, r_total), of channel k at c.p[cur][k * c.cap + r - c_base]
    long long r_total = 0, windows = 0;                      // segments summed, windows decided
    DevFixed<int> d_s[2]; int s_cur = 0;                     // [nchan]: s of the last window decided (-1: none)
    DevFixed<State> d_state; DevFixed<unsigned long long> d_stats;
    DevGrow bits, counts;                                    // one launch's decisions
    fm::EventArena events;                                   // what k_same_frames reports, until the next read
};

namespace {

size_t events_bound(long long nbits) { return (size_t)(nbits / BURST_MIN_BITS + 2) * 2 * EVENT_MAX; }

// room in every channel's arena for the events of nbits more bits
int arena_reserve_bits(nrsc5hip_fm *f, hipStream_t s, long long nbits) { return f->same->events.reserve(s, events_bound(nbits), f->nchan, "SAME"); }

void frames_args(nrsc5hip_fm *f, FramesArgs &g)
{
    SameHost *R = f->same;
    g.targets = nullptr; g.reset_at = nullptr;
    g.state = R->d_state.p; g.stats = R->d_stats.p;
    g.arena = R->events.d_arena; g.used = R->events.d_used.p; g.overflow = R->events.d_used.p + f->nchan; g.arena_cap = R->events.arena_cap;
    g.burst_events = R->burst_events;
}

}  // namespace

void nrsc5::same_free(SameHost *r) { delete r; }

long long nrsc5::same_d_need(const nrsc5hip_fm *f) { return grid_floor(f->same->r_total); }

int nrsc5::same_reset(nrsc5hip_fm *f)
{
    SameHost *R = f->same;
    std::vector<State> init((size_t)f->nchan);
    for (State &st : init) state_init(st);
    std::vector<int> none((size_t)f->nchan, -1);
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpy(R->d_state.p, init.data(), sizeof(State) * f->nchan, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R->d_s[0].p, none.data(), sizeof(int) * f->nchan, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R->d_s[1].p, none.data(), sizeof(int) * f->nchan, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(R->d_stats.p, 0, sizeof(unsigned long long) * NSTATS * f->nchan, f->stream));
    const int rc = R->events.reset(f->stream, f->nchan);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(f->stream));
    R->cur = 0; R->s_cur = 0; R->c_base = 0; R->r_total = 0; R->windows = 0;
    return 0;
}

int nrsc5::same_launch(nrsc5hip_fm *f, hipStream_t s, const float *d, long long m1)
{
    SameHost *R = f->same;
    const long long r1 = segments_total(m1);
    if (r1 <= R->r_total) return 0;
    const long long w1 = windows_total(r1), nwin = w1 - R->windows;
    int rc;
    if ((r1 - R->r_total + TT - 1) / TT > 0x7fffffffLL) FAIL(NRSC5HIP_EINVAL, "push too large (%lld SAME segments)", r1 - R->r_total);
    if ((rc = R->c.reserve(s, r1 - R->c_base, R->r_total - R->c_base, f->nchan, 1, 2048, R->cur, "c"))) return rc;
    if (nwin > 0) {
        if (nwin > 0x7fffffLL) FAIL(NRSC5HIP_EINVAL, "push too large (%lld SAME windows)", nwin);
        if ((rc = R->bits.need((size_t)f->nchan * nwin * BITS_STRIDE)) || (rc = R->counts.need(sizeof(int) * (size_t)f->nchan * nwin))) return rc;
        if ((rc = arena_reserve_bits(f, s, nwin * WIN_MAX_BITS))) return rc;
    }
    TonesArgs t;
    t.d = d; t.d_stride = f->d.cap; t.d_base = f->d_base; t.cs = R->d_cs.p;
    t.c = R->c.p[R->cur]; t.c_stride = R->c.cap; t.c_base = R->c_base; t.r0 = R->r_total; t.r_count = r1 - R->r_total;
    launch_tones(s, (int)((t.r_count + TT - 1) / TT), f->nchan, t);
    HIPCHK(hipGetLastError());
    if (nwin > 0) {
        BitsArgs b;
        b.c = R->c.p[R->cur]; b.c_stride = R->c.cap; b.c_base = R->c_base; b.w0 = R->windows; b.nwin = (int)nwin;
        b.s_in = R->d_s[R->s_cur].p; b.s_out = R->d_s[R->s_cur ^ 1].p;
        b.bits = (uint8_t *)R->bits.p; b.counts = (int *)R->counts.p; b.q = nullptr; b.metric = nullptr; b.s_w = nullptr; b.stats = R->d_stats.p;
        launch_bits(s, f->nchan, b);
        HIPCHK(hipGetLastError());
        FramesArgs g;
        frames_args(f, g);
        g.bits = b.bits; g.chan_stride = nwin * BITS_STRIDE; g.seg_stride = BITS_STRIDE; g.counts = b.counts; g.nseg = (int)nwin;
        launch_frames(s, f->nchan, g);
        HIPCHK(hipGetLastError());
        // what the next call needs of c: the incomplete window
        const long long c_base = w1 * WIN_PTS;
        same::KeepArgs k;
        k.c_old = R->c.p[R->cur]; k.c_new = R->c.p[R->cur ^ 1]; k.c_stride = R->c.cap; k.shift = c_base - R->c_base; k.count = r1 - c_base;
        same::launch_keep(s, f->nchan, k);
        HIPCHK(hipGetLastError());
        R->cur ^= 1; R->s_cur ^= 1; R->c_base = c_base; R->windows = w1;
    }
    R->r_total = r1;
    return 0;
}

#define SAME_ENTER(f)                    \
    FM_FEATURE_ENTER(f, same, "SAME"); \
    SameHost *R = (f)->same

extern "C" int nrsc5hip_fm_same_enable(nrsc5hip_fm *f, const nrsc5hip_same_config *cfg)
{
    FM_ENABLE_CHECK(f, f->same, "SAME");
    if (cfg && (cfg->burst_events < 0 || cfg->burst_events > 1)) FAIL(NRSC5HIP_EINVAL, "burst_events %d: 0 or 1", cfg->burst_events);
    nrsc5::DeviceGuard guard(f->device);
    SameHost *R = new (std::nothrow) SameHost;
    if (!R) FAIL(NRSC5HIP_ENOMEM, "out of host memory");
    if (cfg) R->burst_events = cfg->burst_events;
    R->cs.resize(DEN);
    for (int k = 0; k < DEN; k++) { const double t = 2 * M_PI * k / DEN; R->cs[k] = make_float2((float)cos(t), (float)sin(t)); }
    const size_t K = (size_t)f->nchan;
#define ENABLE_CHK(expr) HIPCHK_OR(expr, delete R)
    ENABLE_CHK(hipMalloc(&R->d_cs.p, sizeof(float2) * DEN));
    ENABLE_CHK(R->c.alloc(2 * WIN_PTS + 8192, f->nchan));
    ENABLE_CHK(hipMalloc(&R->d_s[0].p, sizeof(int) * K));
    ENABLE_CHK(hipMalloc(&R->d_s[1].p, sizeof(int) * K));
    ENABLE_CHK(hipMalloc(&R->d_state.p, sizeof(State) * K));
    ENABLE_CHK(hipMalloc(&R->d_stats.p, sizeof(unsigned long long) * NSTATS * K));
    ENABLE_CHK(R->events.alloc(events_bound(8 * WIN_MAX_BITS * 8), f->nchan));
    ENABLE_CHK(hipMemcpy(R->d_cs.p, R->cs.data(), sizeof(float2) * DEN, hipMemcpyHostToDevice));
#undef ENABLE_CHK
    f->same = R;
    const int rc = same_reset(f);
    if (rc) { f->same = nullptr; delete R; }
    return rc;
}

extern "C" int nrsc5hip_fm_same_info(nrsc5hip_fm *f, int *table, int *points_per_bit, int *window_bits, long long *latency_in)
{
    if (!f) FAIL(NRSC5HIP_EINVAL, "null demodulator");
    if (table) *table = DEN;
    if (points_per_bit) *points_per_bit = S;
    if (window_bits) *window_bits = WIN_BITS;
    if (latency_in) *latency_in = 2 * grid_floor(WIN_PTS + TAIL) - 1;      // the first n_in with (n_in + 1) / 2 >= floor(35721 * 519 / 400)
    return 0;
}

extern "C" int nrsc5hip_fm_same_table(nrsc5hip_fm *f, float *cs)
{
    SAME_ENTER(f);
    if (!cs) FAIL(NRSC5HIP_EINVAL, "null argument");
    memcpy(cs, R->cs.data(), sizeof(float2) * DEN);
    return 0;
}

extern "C" int nrsc5hip_fm_same_read(nrsc5hip_fm *f, nrsc5hip_same_cb cb, void *opaque)
{
    SAME_ENTER(f);
    return R->events.read<Event>(f->stream, f->nchan, "SAME", "k_same_frames",
        [](const Event &ev) { return ev.kind >= NRSC5HIP_SAME_BURST && ev.kind <= NRSC5HIP_SAME_MESSAGE && ev.len <= (unsigned)TEXT_MAX; },
        [&](int c, const Event &ev, const uint8_t *text) { if (cb) cb(opaque, c, ev.kind, ev.first, ev.last, ev.v, text, ev.len); });
}

extern "C" int nrsc5hip_fm_same_get(nrsc5hip_fm *f, int channel, nrsc5hip_same_info *out)
{
    SAME_ENTER(f);
    if (!out || channel < 0 || channel >= f->nchan) FAIL(NRSC5HIP_EINVAL, "bad channel %d", channel);
    HIPCHK(hipStreamSynchronize(f->stream));
    std::vector<State> st(1);
    HIPCHK(hipMemcpy(st.data(), R->d_state.p + channel, sizeof(State), hipMemcpyDeviceToHost));
    const State &s = st[0];
    memset(out, 0, sizeof(*out));
    out->text_len = s.msg_len; out->kind = s.msg_len >= 0 ? s.msg_kind : 0;
    out->first_bit = s.msg_len >= 0 ? s.msg_first : -1; out->last_bit = s.msg_len >= 0 ? s.msg_last : -1;
    if (s.msg_len > 0) memcpy(out->text, s.msg, (size_t)s.msg_len);
    out->group_bursts = s.grp_n; out->group_kind = s.grp_n ? s.grp_kind : 0; out->in_message = s.state == MESSAGE;
    return 0;
}

extern "C" int nrsc5hip_fm_same_stats(nrsc5hip_fm *f, int channel, long long stats[NRSC5HIP_SAME_NSTATS])
{
    SAME_ENTER(f);
    return fm::read_channel_stats<NSTATS>(f, R->d_stats.p, channel, stats);
}

extern "C" int nrsc5hip_stage_same_tones(nrsc5hip_fm *f, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *c_out, float *q_out,
                                         float *metric_out, int32_t *s_out, uint8_t *bits_out, int32_t *counts_out)
{
    SAME_ENTER(f);
    fm::StageFront sf;
    const int rc = sf.open(f, dev_in, in_stride_elems, n_in, false);
    if (rc) return rc;
    const long long m1 = sf.m1, r1 = segments_total(m1), nwin = windows_total(r1);
    const size_t K = (size_t)f->nchan;
    nrsc5::DevTmp c, sk, bits, counts, q, mt, sw;
    HIPCHK(hipMalloc(&c.p, sizeof(float4) * (size_t)(r1 + 1) * K));
    HIPCHK(hipMalloc(&sk.p, sizeof(int) * 2 * K));
    HIPCHK(hipMalloc(&bits.p, (size_t)(nwin + 1) * BITS_STRIDE * K));
    HIPCHK(hipMalloc(&counts.p, sizeof(int) * (size_t)(nwin + 1) * K));
    HIPCHK(hipMalloc(&q.p, sizeof(float) * (size_t)(nwin + 1) * WIN_PTS * K));
    HIPCHK(hipMalloc(&mt.p, sizeof(float) * (size_t)(nwin + 1) * S * K));
    HIPCHK(hipMalloc(&sw.p, sizeof(int) * (size_t)(nwin + 1) * K));
    HIPCHK(hipMemsetAsync(sk.p, 0xff, sizeof(int) * 2 * K, f->stream));
    if (r1 > 0) {
        TonesArgs t;
        t.d = sf.df(); t.d_stride = m1; t.d_base = 0; t.cs = R->d_cs.p;
        t.c = (float4 *)c.p; t.c_stride = r1; t.c_base = 0; t.r0 = 0; t.r_count = r1;
        launch_tones(f->stream, (int)((r1 + TT - 1) / TT), f->nchan, t);
        HIPCHK(hipGetLastError());
    }
    if (nwin > 0) {
        BitsArgs b;
        b.c = (const float4 *)c.p; b.c_stride = r1; b.c_base = 0; b.w0 = 0; b.nwin = (int)nwin;
        b.s_in = (const int *)sk.p; b.s_out = (int *)sk.p + K;
        b.bits = (uint8_t *)bits.p; b.counts = (int *)counts.p; b.q = (float *)q.p; b.metric = (float *)mt.p; b.s_w = (int *)sw.p; b.stats = nullptr;
        launch_bits(f->stream, f->nchan, b);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(f->stream));
    if (c_out && r1 > 0) HIPCHK(hipMemcpy(c_out, c.p, sizeof(float4) * (size_t)r1 * K, hipMemcpyDeviceToHost));
    if (nwin > 0) {
        if (q_out) HIPCHK(hipMemcpy(q_out, q.p, sizeof(float) * (size_t)nwin * WIN_PTS * K, hipMemcpyDeviceToHost));
        if (metric_out) HIPCHK(hipMemcpy(metric_out, mt.p, sizeof(float) * (size_t)nwin * S * K, hipMemcpyDeviceToHost));
        if (s_out) HIPCHK(hipMemcpy(s_out, sw.p, sizeof(int) * (size_t)nwin * K, hipMemcpyDeviceToHost));
        if (bits_out) HIPCHK(hipMemcpy(bits_out, bits.p, (size_t)nwin * BITS_STRIDE * K, hipMemcpyDeviceToHost));
        if (counts_out) HIPCHK(hipMemcpy(counts_out, counts.p, sizeof(int) * (size_t)nwin * K, hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int nrsc5hip_stage_same_frames(nrsc5hip_fm *f, int n, const int *channels, const uint8_t *const *bits, const int *nbits, const int *reset_at)
{
    SAME_ENTER(f);
    if (n < 1 || !bits || !nbits) FAIL(NRSC5HIP_EINVAL, "bad argument");
    int rc = check_targets(f->nchan, n, channels);
    if (rc) return rc;
    long long most = 0;
    for (int i = 0; i < n; i++) {
        if (nbits[i] < 0 || (nbits[i] > 0 && !bits[i])) FAIL(NRSC5HIP_EINVAL, "channel %d of the call: bits missing", i);
        if (reset_at && reset_at[i] > nbits[i]) FAIL(NRSC5HIP_EINVAL, "channel %d of the call: reset behind the end", i);
        most = std::max<long long>(most, nbits[i]);
    }
    const size_t stride = ((size_t)most + 7) & ~(size_t)7;
    std::vector<uint8_t> flat(stride * n + 8, 0);
    std::vector<int> plan(3 * (size_t)n);                    // channel, count, reset_at of every workgroup
    for (int i = 0; i < n; i++) {
        if (nbits[i]) memcpy(flat.data() + stride * i, bits[i], (size_t)nbits[i]);
        plan[i] = channels ? channels[i] : i; plan[n + i] = nbits[i]; plan[2 * n + i] = reset_at ? reset_at[i] : -1;
    }
    // every listed channel gets the room of the longest string, and the channels not listed keep what they have
    if ((rc = arena_reserve_bits(f, f->stream, most))) return rc;
    nrsc5::DevTmp dbits, dplan;
    HIPCHK(hipMalloc(&dbits.p, flat.size()));
    HIPCHK(hipMalloc(&dplan.p, sizeof(int) * plan.size()));
    HIPCHK(hipMemcpyAsync(dbits.p, flat.data(), flat.size(), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(dplan.p, plan.data(), sizeof(int) * plan.size(), hipMemcpyHostToDevice, f->stream));
    FramesArgs g;
    frames_args(f, g);
    g.targets = (const int *)dplan.p; g.counts = (const int *)dplan.p + n; g.reset_at = (const int *)dplan.p + 2 * n;
    g.bits = (const uint8_t *)dbits.p; g.chan_stride = (long long)stride; g.seg_stride = 0; g.nseg = 1;
    launch_frames(f->stream, n, g);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(f->stream));
    return 0;
}
