// RDS / RBDS of the analog host, host side (include/nrsc5hip.h, "RDS"): the tap table in double, the buffers an analog FM object
// gains with nrsc5hip_fm_rds_enable, the launches fm_launch chains behind its front end, the event read-back and the two stage hooks.  The
// kernels are in k_rds.hip; y's buffer that grows, the event arena and the hooks' opening are fm_host.h's.
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
using namespace nrsc5::rds;

struct nrsc5::RdsHost {
    int raw = 0, burst = 2;
    std::vector<float> tab;                                  // host copy [GRID][NT]
    DevFixed<float> d_tab;                                   // [NT][GRID], indexed by r mod GRID
    fm::PingPong<float2> y; long long y_base = 0; int cur = 0;   // y[r], r in [y_base, r_total), of channel c at y.p[cur][c * y.cap + r - y_base]
    long long r_total = 0, windows = 0;                      // grid points summed, windows decided
    DevFixed<int> d_s[2]; int s_cur = 0;                     // [nchan]: s of the last window decided (-1: none)
    DevFixed<State> d_state; DevFixed<unsigned long long> d_stats;
    DevGrow bits, counts;                                    // one launch's decisions
    fm::EventArena events;                                   // what k_rds_groups reports, until the next read
};

namespace {

using fm::sinc;
double shape_h(double t, double T) { return sinc(4 * t / T + 0.5) + sinc(4 * t / T - 0.5); }

// tab[ph][j]: the biphase symbol, centred on the grid point, tau = j - HALF - ph / GRID samples from it, under the Hann window over |tau| <= 2 T
std::vector<float> design_taps()
{
    const double T = (double)DEN / 38.0;
    std::vector<float> tab((size_t)GRID * NT);
    for (int ph = 0; ph < GRID; ph++)
        for (int j = 0; j < NT; j++) {
            const double tau = (double)(j - HALF) - (double)ph / GRID, t = tau + T / 4;
            const double g = shape_h(t, T) - shape_h(t - T / 2, T);
            const double w = fabs(tau) <= 2 * T ? 0.5 * (1 + cos(M_PI * tau / (2 * T))) : 0.0;
            tab[(size_t)ph * NT + j] = (float)(g * w);
        }
    return tab;
}

size_t events_bound(long long nbits) { return (size_t)(nbits / 104 + 2) * EVENTS_PER_GROUP * EVENT_MAX; }

// room in every channel's arena for the events of nbits more bits
int arena_reserve_bits(nrsc5hip_fm *f, hipStream_t s, long long nbits) { return f->rds->events.reserve(s, events_bound(nbits), f->nchan, "RDS"); }

void groups_args(nrsc5hip_fm *f, GroupsArgs &g)
{
    RdsHost *R = f->rds;
    g.targets = nullptr; g.reset_at = nullptr;
    g.state = R->d_state.p; g.stats = R->d_stats.p;
    g.arena = R->events.d_arena; g.used = R->events.d_used.p; g.overflow = R->events.d_used.p + f->nchan; g.arena_cap = R->events.arena_cap;
    g.raw = R->raw; g.burst = R->burst;
}

}  // namespace

void nrsc5::rds_free(RdsHost *r) { delete r; }

long long nrsc5::rds_d_need(const nrsc5hip_fm *f)
{
    const long long m = ((long long)DEN * f->rds->r_total) / GRID - HALF;
    return m < 0 ? 0 : m;
}

int nrsc5::rds_reset(nrsc5hip_fm *f)
{
    RdsHost *R = f->rds;
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
    R->cur = 0; R->s_cur = 0; R->y_base = 0; R->r_total = 0; R->windows = 0;
    return 0;
}

int nrsc5::rds_launch(nrsc5hip_fm *f, hipStream_t s, const float *d, long long m1)
{
    RdsHost *R = f->rds;
    const long long r1 = points_total(m1);
    if (r1 <= R->r_total) return 0;
    const long long w1 = r1 / WIN_PTS, nwin = w1 - R->windows;
    int rc;
    if ((rc = R->y.reserve(s, r1 - R->y_base, R->r_total - R->y_base, f->nchan, 1, 2048, R->cur, "y"))) return rc;
    if (nwin > 0) {
        if (nwin > 0x7fffffLL) FAIL(NRSC5HIP_EINVAL, "push too large (%lld RDS windows)", nwin);
        if ((rc = R->bits.need((size_t)f->nchan * nwin * BITS_STRIDE)) || (rc = R->counts.need(sizeof(int) * (size_t)f->nchan * nwin))) return rc;
        if ((rc = arena_reserve_bits(f, s, nwin * WIN_MAX_BITS))) return rc;
    }
    MfArgs m;
    m.d = d; m.d_stride = f->d.cap; m.d_base = f->d_base; m.cs = f->d_cs; m.tab = R->d_tab.p;
    m.y = R->y.p[R->cur]; m.y_stride = R->y.cap; m.y_base = R->y_base; m.r0 = R->r_total; m.r_count = r1 - R->r_total;
    launch_mf(s, (int)((m.r_count + MT - 1) / MT), f->nchan, m);
    HIPCHK(hipGetLastError());
    if (nwin > 0) {
        BitsArgs b;
        b.y = R->y.p[R->cur]; b.y_stride = R->y.cap; b.y_base = R->y_base; b.w0 = R->windows; b.nwin = (int)nwin;
        b.s_in = R->d_s[R->s_cur].p; b.s_out = R->d_s[R->s_cur ^ 1].p;
        b.bits = (uint8_t *)R->bits.p; b.counts = (int *)R->counts.p; b.energy = nullptr; b.s_w = nullptr; b.stats = R->d_stats.p;
        launch_bits(s, f->nchan, b);
        HIPCHK(hipGetLastError());
        GroupsArgs g;
        groups_args(f, g);
        g.bits = b.bits; g.chan_stride = nwin * BITS_STRIDE; g.seg_stride = BITS_STRIDE; g.counts = b.counts; g.nseg = (int)nwin;
        launch_groups(s, f->nchan, g);
        HIPCHK(hipGetLastError());
        // what the next call needs of y: the incomplete window and, for its first decision, the 8 points in front of it
        const long long y_base = w1 * WIN_PTS - S;
        rds::KeepArgs k;
        k.y_old = R->y.p[R->cur]; k.y_new = R->y.p[R->cur ^ 1]; k.y_stride = R->y.cap; k.shift = y_base - R->y_base; k.count = r1 - y_base;
        rds::launch_keep(s, f->nchan, k);
        HIPCHK(hipGetLastError());
        R->cur ^= 1; R->s_cur ^= 1; R->y_base = y_base; R->windows = w1;
    }
    R->r_total = r1;
    return 0;
}

#define RDS_ENTER(f)                   \
    FM_FEATURE_ENTER(f, rds, "RDS"); \
    RdsHost *R = (f)->rds

extern "C" int nrsc5hip_fm_rds_enable(nrsc5hip_fm *f, const nrsc5hip_rds_config *cfg)
{
    FM_ENABLE_CHECK(f, f->rds, "RDS");
    if (cfg && (cfg->correct_burst < 0 || cfg->correct_burst > 2)) FAIL(NRSC5HIP_EINVAL, "correct_burst %d: 0 .. 2", cfg->correct_burst);
    nrsc5::DeviceGuard guard(f->device);
    RdsHost *R = new (std::nothrow) RdsHost;
    if (!R) FAIL(NRSC5HIP_ENOMEM, "out of host memory");
    if (cfg) { R->raw = cfg->raw_groups != 0; R->burst = cfg->correct_burst; }
    R->tab = design_taps();
    std::vector<float> dev((size_t)NT * GRID);
    for (int q = 0; q < GRID; q++) {
        const int ph = (int)(((long long)DEN * q) % GRID);
        for (int j = 0; j < NT; j++) dev[(size_t)j * GRID + q] = R->tab[(size_t)ph * NT + j];
    }
    const size_t K = (size_t)f->nchan;
#define ENABLE_CHK(expr) HIPCHK_OR(expr, delete R)
    ENABLE_CHK(hipMalloc(&R->d_tab.p, sizeof(float) * dev.size()));
    ENABLE_CHK(R->y.alloc(2 * WIN_PTS + 8192, f->nchan));
    ENABLE_CHK(hipMalloc(&R->d_s[0].p, sizeof(int) * K));
    ENABLE_CHK(hipMalloc(&R->d_s[1].p, sizeof(int) * K));
    ENABLE_CHK(hipMalloc(&R->d_state.p, sizeof(State) * K));
    ENABLE_CHK(hipMalloc(&R->d_stats.p, sizeof(unsigned long long) * NSTATS * K));
    ENABLE_CHK(R->events.alloc(events_bound(4 * WIN_MAX_BITS * 8), f->nchan));
    ENABLE_CHK(hipMemcpy(R->d_tab.p, dev.data(), sizeof(float) * dev.size(), hipMemcpyHostToDevice));
#undef ENABLE_CHK
    f->rds = R;
    const int rc = rds_reset(f);
    if (rc) { f->rds = nullptr; delete R; }
    return rc;
}

extern "C" int nrsc5hip_fm_rds_info(nrsc5hip_fm *f, int *taps, int *phases, int *points_per_bit, int *window_bits, long long *latency_in)
{
    if (!f) FAIL(NRSC5HIP_EINVAL, "null demodulator");
    if (taps) *taps = NT;
    if (phases) *phases = GRID;
    if (points_per_bit) *points_per_bit = S;
    if (window_bits) *window_bits = WIN_BITS;
    if (latency_in) *latency_in = 2 * (((long long)DEN * (WIN_PTS - 1)) / GRID + HALF + 1) - 1;
    return 0;
}

extern "C" int nrsc5hip_fm_rds_taps(nrsc5hip_fm *f, float *taps)
{
    RDS_ENTER(f);
    if (!taps) FAIL(NRSC5HIP_EINVAL, "null argument");
    memcpy(taps, R->tab.data(), sizeof(float) * R->tab.size());
    return 0;
}

extern "C" int nrsc5hip_fm_rds_read(nrsc5hip_fm *f, nrsc5hip_rds_cb cb, void *opaque)
{
    RDS_ENTER(f);
    return R->events.read<Event>(f->stream, f->nchan, "RDS", "k_rds_groups",
        [](const Event &ev) { return ev.kind >= NRSC5HIP_RDS_PI && ev.kind <= NRSC5HIP_RDS_GROUP && ev.len <= 64; },
        [&](int c, const Event &ev, const uint8_t *text) { if (cb) cb(opaque, c, ev.kind, ev.group, ev.bit, ev.v, text, ev.len); });
}

extern "C" int nrsc5hip_fm_rds_get(nrsc5hip_fm *f, int channel, nrsc5hip_rds_info *out)
{
    RDS_ENTER(f);
    if (!out || channel < 0 || channel >= f->nchan) FAIL(NRSC5HIP_EINVAL, "bad channel %d", channel);
    HIPCHK(hipStreamSynchronize(f->stream));
    State st;
    HIPCHK(hipMemcpy(&st, R->d_state.p + channel, sizeof(st), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    out->pi = st.pi; out->pty = st.pty; out->tp = st.tp; out->ta = st.ta; out->ms = st.ms; out->di = st.di; out->synced = st.synced;
    out->ps_len = st.ps_have ? 8 : -1;
    if (st.ps_have) memcpy(out->ps, st.ps_last, 8);
    out->rt_len = st.rt_have ? st.rt_last_len : -1; out->rt_ab = st.rt_ab;
    if (st.rt_have) memcpy(out->rt, st.rt_last, (size_t)st.rt_last_len);
    out->have_clock = st.clk_have; out->mjd = st.clk[0]; out->hour = st.clk[1]; out->minute = st.clk[2]; out->offset_half_hours = st.clk[3];
    return 0;
}

extern "C" int nrsc5hip_fm_rds_stats(nrsc5hip_fm *f, int channel, long long stats[NRSC5HIP_RDS_NSTATS])
{
    RDS_ENTER(f);
    return fm::read_channel_stats<NSTATS>(f, R->d_stats.p, channel, stats);
}

extern "C" int nrsc5hip_stage_rds_mf(nrsc5hip_fm *f, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *y_out, float *energy_out,
                                     int32_t *s_out, uint8_t *bits_out, int32_t *counts_out)
{
    RDS_ENTER(f);
    fm::StageFront sf;
    const int rc = sf.open(f, dev_in, in_stride_elems, n_in, false);
    if (rc) return rc;
    const long long m1 = sf.m1, r1 = points_total(m1), nwin = r1 / WIN_PTS;
    const size_t K = (size_t)f->nchan;
    nrsc5::DevTmp y, sk, bits, counts, en, sw;
    HIPCHK(hipMalloc(&y.p, sizeof(float2) * (size_t)(r1 + 1) * K));
    HIPCHK(hipMalloc(&sk.p, sizeof(int) * 2 * K));
    HIPCHK(hipMalloc(&bits.p, (size_t)(nwin + 1) * BITS_STRIDE * K));
    HIPCHK(hipMalloc(&counts.p, sizeof(int) * (size_t)(nwin + 1) * K));
    HIPCHK(hipMalloc(&en.p, sizeof(float) * (size_t)(nwin + 1) * S * K));
    HIPCHK(hipMalloc(&sw.p, sizeof(int) * (size_t)(nwin + 1) * K));
    HIPCHK(hipMemsetAsync(sk.p, 0xff, sizeof(int) * 2 * K, f->stream));
    if (r1 > 0) {
        MfArgs m;
        m.d = sf.df(); m.d_stride = m1; m.d_base = 0; m.cs = f->d_cs; m.tab = R->d_tab.p;
        m.y = (float2 *)y.p; m.y_stride = r1; m.y_base = 0; m.r0 = 0; m.r_count = r1;
        launch_mf(f->stream, (int)((r1 + MT - 1) / MT), f->nchan, m);
        HIPCHK(hipGetLastError());
    }
    if (nwin > 0) {
        BitsArgs b;
        b.y = (const float2 *)y.p; b.y_stride = r1; b.y_base = 0; b.w0 = 0; b.nwin = (int)nwin;
        b.s_in = (const int *)sk.p; b.s_out = (int *)sk.p + K;
        b.bits = (uint8_t *)bits.p; b.counts = (int *)counts.p; b.energy = (float *)en.p; b.s_w = (int *)sw.p; b.stats = nullptr;
        launch_bits(f->stream, f->nchan, b);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(f->stream));
    if (y_out && r1 > 0) HIPCHK(hipMemcpy(y_out, y.p, sizeof(float2) * (size_t)r1 * K, hipMemcpyDeviceToHost));
    if (nwin > 0) {
        if (energy_out) HIPCHK(hipMemcpy(energy_out, en.p, sizeof(float) * (size_t)nwin * S * K, hipMemcpyDeviceToHost));
        if (s_out) HIPCHK(hipMemcpy(s_out, sw.p, sizeof(int) * (size_t)nwin * K, hipMemcpyDeviceToHost));
        if (bits_out) HIPCHK(hipMemcpy(bits_out, bits.p, (size_t)nwin * BITS_STRIDE * K, hipMemcpyDeviceToHost));
        if (counts_out) HIPCHK(hipMemcpy(counts_out, counts.p, sizeof(int) * (size_t)nwin * K, hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int nrsc5hip_stage_rds_groups(nrsc5hip_fm *f, int n, const int *channels, const uint8_t *const *bits, const int *nbits, const int *reset_at)
{
    RDS_ENTER(f);
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
    GroupsArgs g;
    groups_args(f, g);
    g.targets = (const int *)dplan.p; g.counts = (const int *)dplan.p + n; g.reset_at = (const int *)dplan.p + 2 * n;
    g.bits = (const uint8_t *)dbits.p; g.chan_stride = (long long)stride; g.seg_stride = 0; g.nseg = 1;
    launch_groups(f->stream, n, g);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(f->stream));
    return 0;
}
