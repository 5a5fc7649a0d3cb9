// Analog FM audio, host side (include/nrsc5hip.h, "analog FM audio"): the filter design in double, the object's buffers, the push (fm_launch) and
// the C ABI, reception steering included.  The kernels are in k_fm_audio.hip; the object and the plumbing the analog units share are in fm_host.h;
// the definition is DESIGN.md (o).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "nrsc5hip.h"
#include "host_util.h"
#include "fm_host.h"

using namespace nrsc5::fm;

namespace {

constexpr double FS = 744187.5, FS1 = FS / 2;
constexpr double PASS_A = 95e3, STOP_A = 129361.0, ATT_A = 80.0;     // channel filter: passband edge, first primary-main carrier, design target
constexpr double PASS_B = 15e3, STOP_B = 19e3, ATT_B = 66.0;          // audio prototype at 16 Fs1
constexpr double PASS_N = 4e3, STOP_N = 8e3;                          // the narrow prototype of reception steering: the same transition width
constexpr double EQ_F0 = 28000.0, EQ_F1 = 48000.0;                    // the droop equaliser is exact at these two frequencies
constexpr int MAX_CHANNELS = 512;
constexpr long long KEEP_MAX_BLOCKS = 2 * W + 3;

// Kaiser-windowed sinc, fc in cycles per sample, symmetric about (taps - 1) / 2
std::vector<double> kaiser_lowpass(int taps, double fc, double att_db)
{
    const double beta = 0.1102 * (att_db - 8.7), i0b = bessel_i0(beta);
    std::vector<double> h(taps);
    for (int i = 0; i < taps; i++) {
        const double tau = i - 0.5 * (taps - 1), u = 2.0 * tau / (taps - 1);
        const double w = fabs(u) < 1.0 ? bessel_i0(beta * sqrt(1.0 - u * u)) / i0b : (fabs(u) == 1.0 ? 1.0 / i0b : 0.0);
        h[i] = 2.0 * fc * sinc(2.0 * fc * tau) * w;
    }
    return h;
}

// audio prototype at 16 Fs1 with the given pass and stop edge: Kaiser lowpass convolved with the sampled one-pole, DC gain 16 -> [PHASES][tb]
std::vector<float> audio_prototype(double pass, double stop, double deemphasis_us, int *tb_out)
{
    const double fv = PHASES * FS1, dw = 2 * M_PI * (stop - pass) / fv;
    const int nk = (int)ceil((ATT_B - 7.95) / (2.285 * dw)) + 1;
    std::vector<double> g = kaiser_lowpass(nk, 0.5 * (pass + stop) / fv, ATT_B);
    if (deemphasis_us > 0) {
        const double tf = deemphasis_us * 1e-6 * fv;
        const int ne = (int)ceil(30.0 * log(2.0) * tf);                 // exp(-v / tf) < 2^-30 from here on
        std::vector<double> e(ne), y(nk + ne - 1, 0.0);
        for (int v = 0; v < ne; v++) e[v] = exp(-v / tf);
        e[0] = 0.5;                                                     // the step at t = 0 sampled at its mid value
        for (int i = 0; i < nk; i++)
            for (int v = 0; v < ne; v++) y[i + v] += g[i] * e[v];
        g.swap(y);
    }
    double sum = 0;
    for (double v : g) sum += v;
    const int tb = ((int)g.size() + PHASES - 1) / PHASES;
    std::vector<float> tab((size_t)PHASES * tb, 0.0f);
    for (size_t v = 0; v < g.size(); v++) tab[(v % PHASES) * tb + v / PHASES] = (float)(g[v] * PHASES / sum);
    *tb_out = tb;
    return tab;
}

// [PHASES][tb] -> [tb][PHASES], as the kernel reads it
std::vector<float> device_layout(const std::vector<float> &tab, int tb)
{
    std::vector<float> dev((size_t)PHASES * tb);
    for (int p = 0; p < PHASES; p++)
        for (int j = 0; j < tb; j++) dev[(size_t)j * PHASES + p] = tab[(size_t)p * tb + j];
    return dev;
}

void free_fm(nrsc5hip_fm *f)
{
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    (void)hipFree(f->d_ha); (void)hipFree(f->d_tab); (void)hipFree(f->d_win); (void)hipFree(f->d_scale); (void)hipFree(f->d_pilot); (void)hipFree(f->d_cs);
    (void)hipFree(f->d_hist[0]); (void)hipFree(f->d_hist[1]);
    (void)hipFree(f->d_clips); (void)hipFree(f->d_tab_n); (void)hipFree(f->d_steer);
    nrsc5::rds_free(f->rds);
    nrsc5::same_free(f->same);
    nrsc5::carrier_free(f->carrier);
    nrsc5::impair_free(f->impair);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

int fm_zero_state(nrsc5hip_fm *f)
{
    HIPCHK(hipMemsetAsync(f->d_hist[0], 0, sizeof(int) * HIST * f->nchan, f->stream));
    HIPCHK(hipMemsetAsync(f->d_hist[1], 0, sizeof(int) * HIST * f->nchan, f->stream));
    HIPCHK(hipMemsetAsync(f->d_clips, 0, sizeof(unsigned long long) * 2 * f->nchan, f->stream));
    HIPCHK(hipMemsetAsync(f->d_pilot, 0, sizeof(float) * 2 * f->nchan, f->stream));
    if (f->d_steer) HIPCHK(hipMemsetAsync(f->d_steer, 0, sizeof(float4) * f->nchan, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    f->cur = 0; f->n_total = 0; f->m_total = 0; f->blocks = 0; f->audio_blocks = 0; f->d_base = 0; f->p_base = 0; f->launches = 0;
    if (f->carrier) { const int rc = nrsc5::carrier_reset(f); if (rc) return rc; }
    if (f->impair) { const int rc = nrsc5::impair_reset(f); if (rc) return rc; }
    if (f->same) { const int rc = nrsc5::same_reset(f); if (rc) return rc; }
    return f->rds ? nrsc5::rds_reset(f) : 0;
}

struct Counts { long long n1, m1, b1, a1; };
Counts counts_after(const nrsc5hip_fm *f, long long n_in)
{
    Counts c;
    c.n1 = f->n_total + n_in; c.m1 = (c.n1 + 1) >> 1; c.b1 = c.m1 / BLOCK; c.a1 = c.b1 > W ? c.b1 - W : 0;
    return c;
}

// room for d[d_base, m1) and p[p_base, b1)
int fm_reserve(nrsc5hip_fm *f, hipStream_t s, long long m1, long long b1)
{
    const int rc = f->d.reserve(s, m1 - f->d_base, f->m_total - f->d_base, f->nchan, 1, 4096, f->cur, "d");
    return rc ? rc : f->p.reserve(s, b1 - f->p_base, f->blocks - f->p_base, f->nchan, 1, 64, f->cur, "pilot sums");
}

}  // namespace

thread_local long long *nrsc5::fm::launch_count = nullptr;

double nrsc5::fm::bessel_i0(double x)
{
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 500; k++) {
        t *= (x / (2.0 * k)) * (x / (2.0 * k));
        s += t;
        if (t < 1e-18 * s) break;
    }
    return s;
}

int nrsc5::fm_nchan(const nrsc5hip_fm *f) { return f->nchan; }
int nrsc5::fm_device(const nrsc5hip_fm *f) { return f->device; }

int nrsc5::fm_check_input(const nrsc5hip_fm *f, const void *dev_in, long long in_stride_elems, long long n_in)
{
    if (n_in < 0 || (n_in > 0 && !dev_in)) FAIL(NRSC5HIP_EINVAL, "bad input (n_in %lld)", n_in);
    if (((uintptr_t)dev_in & 3) || (in_stride_elems & 1)) FAIL(NRSC5HIP_EINVAL, "input not aligned to 4 bytes (in_stride_elems %lld)", in_stride_elems);
    if (f->nchan > 1 && in_stride_elems < 2 * n_in) FAIL(NRSC5HIP_EINVAL, "in_stride_elems %lld < 2 * n_in %lld", in_stride_elems, n_in);
    return 0;
}

int nrsc5::fm_check(nrsc5hip_fm *f, long long n_in, const int16_t *dev_out, long long out_stride_elems, long long out_capacity, long long *n_out)
{
    const Counts c = counts_after(f, n_in);
    const long long nout = BLOCK_OUT * (c.a1 - f->audio_blocks);
    if (nout > 0 && !dev_out) FAIL(NRSC5HIP_EINVAL, "null output");
    if (out_capacity < 0 || (f->nchan > 1 && out_stride_elems < 2 * out_capacity))
        FAIL(NRSC5HIP_EINVAL, "out_stride_elems %lld < 2 * out_capacity %lld", out_stride_elems, out_capacity);
    if (nout > out_capacity) FAIL(NRSC5HIP_EOVERFLOW, "push of %lld samples yields %lld audio frames per channel > out_capacity %lld", n_in, nout, out_capacity);
    if ((c.m1 - f->m_total + FT - 1) / FT > 0x7fffffffLL) FAIL(NRSC5HIP_EINVAL, "push too large (%lld samples)", n_in);
    if (n_out) *n_out = nout;
    return 0;
}

// front, pilot sums, audio, the carrier sums and report (when enabled; steered, the sums in front of the audio; the impairment sums and report
// between the two) and the kept tails on `stream`; no host wait (but for a buffer that has to grow)
int nrsc5::fm_launch(nrsc5hip_fm *f, hipStream_t s, const int16_t *dev_in, long long in_stride, long long n_in, int16_t *out, long long out_stride)
{
    if (n_in <= 0) return 0;
    f->processed = true;
    CountLaunches counting(&f->launches);
    const Counts c = counts_after(f, n_in);
    int rc = fm_reserve(f, s, c.m1, c.b1);
    if (rc) return rc;
    if (f->carrier && (rc = nrsc5::carrier_reserve(f, s, c.m1, c.b1))) return rc;
    if (f->impair && (rc = nrsc5::impair_reserve(f, s, c.b1))) return rc;
    float *d = f->d.p[f->cur]; float2 *p = f->p.p[f->cur];
    if (c.m1 > f->m_total) {
        FrontArgs a;
        a.in = dev_in; a.in_stride = in_stride; a.n0 = f->n_total; a.n_in = n_in; a.hist = f->d_hist[f->cur]; a.ha = f->d_ha;
        a.d = d; a.d_stride = f->d.cap; a.d_base = f->d_base; a.m0 = f->m_total; a.m_count = c.m1 - f->m_total;
        if (f->carrier) { const nrsc5::FrontTarget t = nrsc5::carrier_front(f); a.r = t.r; a.r_stride = t.r_stride; a.r_base = t.r_base; }
        launch_front(s, (int)((a.m_count + FT - 1) / FT), f->nchan, a);
        HIPCHK(hipGetLastError());
    }
    if (f->rds && (rc = nrsc5::rds_launch(f, s, d, c.m1))) return rc;
    if (f->same && (rc = nrsc5::same_launch(f, s, d, c.m1))) return rc;
    if (c.b1 > f->blocks) {
        PilotArgs a;
        a.d = d; a.d_stride = f->d.cap; a.d_base = f->d_base; a.cs = f->d_cs; a.p = p; a.p_stride = f->p.cap; a.p_base = f->p_base; a.j0 = f->blocks;
        launch_pilot(s, (int)(c.b1 - f->blocks), f->nchan, a);
        HIPCHK(hipGetLastError());
    }
    const bool new_blocks = f->carrier && c.b1 > f->blocks;
    if (f->steer && new_blocks && (rc = nrsc5::carrier_launch_sums(f, s, d, c.b1))) return rc;      // steered: the audio reads the new blocks' triples
    if (c.a1 > f->audio_blocks) {
        SteeredAudioArgs a;
        a.d = d; a.d_stride = f->d.cap; a.d_base = f->d_base; a.p = p; a.p_stride = f->p.cap; a.p_base = f->p_base; a.cs = f->d_cs;
        a.tab = f->d_tab; a.tb = f->tb; a.win = f->d_win; a.wsum = f->wsum; a.aq = f->aq; a.bq = f->bq; a.pilot_min = f->pilot_min; a.scale = f->d_scale;
        a.j0 = f->audio_blocks; a.k0 = BLOCK_OUT * f->audio_blocks; a.out = out; a.out_stride = out_stride; a.clips = f->d_clips; a.pilot = f->d_pilot;
        if (f->steer) {
            const nrsc5::Triples t = nrsc5::carrier_triples(f);
            a.t = t.t; a.t_stride = t.t_stride; a.t_base = t.t_base; a.tab_n = f->d_tab_n; a.ramps = f->ramps; a.steer = f->d_steer; a.steer_stride = 1; a.steer_every = 0;
            launch_audio_steered(s, (int)(c.a1 - f->audio_blocks), f->nchan, a);
        } else launch_audio(s, (int)(c.a1 - f->audio_blocks), f->nchan, a);
        HIPCHK(hipGetLastError());
    }
    if (!f->steer && new_blocks && (rc = nrsc5::carrier_launch_sums(f, s, d, c.b1))) return rc;
    if (f->impair && new_blocks && (rc = nrsc5::impair_launch(f, s, d, c.b1, c.a1))) return rc;       // reads this push's r: in front of its hand-over
    if (new_blocks && (rc = nrsc5::carrier_launch_report(f, s, c.m1, c.b1, c.a1))) return rc;
    // what the next call needs: d from the first tap of audio block a1, the block sums from a1 - W, the last HIST input samples
    long long d_base = (long long)BLOCK * c.a1 - f->tb - 1, p_base = c.a1 - W;
    if (d_base < 0) d_base = 0;
    if (p_base < 0) p_base = 0;
    if (f->rds && nrsc5::rds_d_need(f) < d_base) d_base = nrsc5::rds_d_need(f);     // ... and d from the first tap of the first grid point not yet summed
    if (f->same && nrsc5::same_d_need(f) < d_base) d_base = nrsc5::same_d_need(f);  // ... and from the first SAME segment not yet summed
    KeepArgs k;
    k.d_old = d; k.d_new = f->d.p[f->cur ^ 1]; k.d_stride = f->d.cap; k.d_shift = d_base - f->d_base; k.d_count = c.m1 - d_base;
    k.p_old = p; k.p_new = f->p.p[f->cur ^ 1]; k.p_stride = f->p.cap; k.p_shift = p_base - f->p_base; k.p_count = c.b1 - p_base;
    k.in = dev_in; k.in_stride = in_stride; k.n0 = f->n_total; k.n_in = n_in; k.hist_old = f->d_hist[f->cur]; k.hist_new = f->d_hist[f->cur ^ 1];
    launch_keep(s, f->nchan, k);
    HIPCHK(hipGetLastError());
    f->cur ^= 1; f->d_base = d_base; f->p_base = p_base;
    f->n_total = c.n1; f->m_total = c.m1; f->blocks = c.b1; f->audio_blocks = c.a1;
    return 0;
}

extern "C" int nrsc5hip_fm_create(const nrsc5hip_fm_config *cfg, nrsc5hip_fm **out)
{
    if (!cfg || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->nchan < 1 || cfg->nchan > MAX_CHANNELS) FAIL(NRSC5HIP_EINVAL, "nchan %d out of range 1..%d", cfg->nchan, MAX_CHANNELS);
    if (cfg->deemphasis_us != 75.0 && cfg->deemphasis_us != 50.0 && cfg->deemphasis_us != 0.0)
        FAIL(NRSC5HIP_EINVAL, "deemphasis_us %g: 75, 50 or 0", cfg->deemphasis_us);
    if (!(cfg->pilot_min >= 0.0) || !(cfg->pilot_min <= 1.0)) FAIL(NRSC5HIP_EINVAL, "pilot_min %g outside 0..1", cfg->pilot_min);
    for (int k = 0; k < cfg->nchan; k++)
        if (cfg->gain && !std::isfinite(cfg->gain[k])) FAIL(NRSC5HIP_EINVAL, "channel %d: gain not finite", k);

    nrsc5hip_fm *f = new (std::nothrow) nrsc5hip_fm;
    if (!f) FAIL(NRSC5HIP_ENOMEM, "out of host memory");
    f->device = cfg->device; f->nchan = cfg->nchan; f->deemphasis_us = cfg->deemphasis_us;
    f->pilot_min = cfg->pilot_min == 0.0 ? 0.03f : (float)cfg->pilot_min;
    for (int k = 0; k < cfg->nchan; k++) f->scale.push_back((float)(32767.0 * (cfg->gain ? cfg->gain[k] : 1.0f)));
    {   // channel filter, DC gain 1
        std::vector<double> h = kaiser_lowpass(TA, 0.5 * (PASS_A + STOP_A) / FS, ATT_A);
        double sum = 0;
        for (double v : h) sum += v;
        for (double v : h) f->ha.push_back((float)(v / sum));
    }
    {   // droop equaliser (a, b, a): b + 2 a cos(w) = 1 / sinc(f / Fs1) at EQ_F0 and EQ_F1
        const double r0 = 1.0 / sinc(EQ_F0 / FS1), r1 = 1.0 / sinc(EQ_F1 / FS1), c0 = cos(2 * M_PI * EQ_F0 / FS1), c1 = cos(2 * M_PI * EQ_F1 / FS1);
        const double a = (r0 - r1) / (2 * (c0 - c1));
        f->aq = (float)a; f->bq = (float)(r0 - 2 * a * c0);
    }
    f->tab = audio_prototype(PASS_B, STOP_B, cfg->deemphasis_us, &f->tb);
    const std::vector<float> dev_tab = device_layout(f->tab, f->tb);
    const std::vector<float> win = hann_window();
    double wsum = 0;
    for (int w = -W; w <= W; w++) wsum += hann(w);           // of the window in double: what the audio kernel divides by
    f->wsum = (float)wsum;
    std::vector<float2> cs(PILOT_DEN);
    for (int k = 0; k < PILOT_DEN; k++) { const double t = 2 * M_PI * k / PILOT_DEN; cs[k] = make_float2((float)cos(t), (float)sin(t)); }

    nrsc5::DeviceGuard guard(f->device);
#define CREATE_CHK(expr) HIPCHK_OR(expr, free_fm(f))
    CREATE_CHK(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    CREATE_CHK(hipMalloc(&f->d_ha, sizeof(float) * TA));
    CREATE_CHK(hipMalloc(&f->d_tab, sizeof(float) * dev_tab.size()));
    CREATE_CHK(hipMalloc(&f->d_win, sizeof(float) * win.size()));
    CREATE_CHK(hipMalloc(&f->d_scale, sizeof(float) * f->nchan));
    CREATE_CHK(hipMalloc(&f->d_pilot, sizeof(float) * 2 * f->nchan));
    CREATE_CHK(hipMalloc(&f->d_cs, sizeof(float2) * PILOT_DEN));
    CREATE_CHK(hipMalloc(&f->d_hist[0], sizeof(int) * HIST * f->nchan));
    CREATE_CHK(hipMalloc(&f->d_hist[1], sizeof(int) * HIST * f->nchan));
    CREATE_CHK(hipMalloc(&f->d_clips, sizeof(unsigned long long) * 2 * f->nchan));
    CREATE_CHK(f->d.alloc(KEEP_MAX_BLOCKS * BLOCK + f->tb + 65536, f->nchan));
    CREATE_CHK(f->p.alloc(KEEP_MAX_BLOCKS + 256, f->nchan));
    CREATE_CHK(hipMemcpy(f->d_ha, f->ha.data(), sizeof(float) * TA, hipMemcpyHostToDevice));
    CREATE_CHK(hipMemcpy(f->d_tab, dev_tab.data(), sizeof(float) * dev_tab.size(), hipMemcpyHostToDevice));
    CREATE_CHK(hipMemcpy(f->d_win, win.data(), sizeof(float) * win.size(), hipMemcpyHostToDevice));
    CREATE_CHK(hipMemcpy(f->d_scale, f->scale.data(), sizeof(float) * f->nchan, hipMemcpyHostToDevice));
    CREATE_CHK(hipMemcpy(f->d_cs, cs.data(), sizeof(float2) * PILOT_DEN, hipMemcpyHostToDevice));
#undef CREATE_CHK
    int rc = fm_zero_state(f);
    if (rc) { free_fm(f); return rc; }
    *out = f;
    return 0;
}

extern "C" void nrsc5hip_fm_destroy(nrsc5hip_fm *f)
{
    if (!f) return;
    nrsc5::DeviceGuard guard(f->device);
    free_fm(f);
}

extern "C" int nrsc5hip_fm_reset(nrsc5hip_fm *f)
{
    if (!f) FAIL(NRSC5HIP_EINVAL, "null demodulator");
    nrsc5::DeviceGuard guard(f->device);
    HIPCHK(hipStreamSynchronize(f->stream));
    return fm_zero_state(f);
}

extern "C" int nrsc5hip_fm_info(nrsc5hip_fm *f, int *taps_channel, int *taps_audio, int *phases, long long *latency_in)
{
    if (!f) FAIL(NRSC5HIP_EINVAL, "null demodulator");
    if (taps_channel) *taps_channel = TA;
    if (taps_audio) *taps_audio = f->tb;
    if (phases) *phases = PHASES;
    if (latency_in) *latency_in = 2LL * BLOCK * (W + 1) - 1;
    return 0;
}

extern "C" int nrsc5hip_fm_taps(nrsc5hip_fm *f, float *channel, float *audio)
{
    if (!f || (!channel && !audio)) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (channel) memcpy(channel, f->ha.data(), sizeof(float) * TA);
    if (audio) memcpy(audio, f->tab.data(), sizeof(float) * f->tab.size());
    return 0;
}

extern "C" long long nrsc5hip_fm_outputs_for(nrsc5hip_fm *f, long long n_in)
{
    if (!f) FAIL(NRSC5HIP_EINVAL, "null demodulator");
    if (n_in < 0) FAIL(NRSC5HIP_EINVAL, "n_in %lld negative", n_in);
    return BLOCK_OUT * (counts_after(f, n_in).a1 - f->audio_blocks);
}

extern "C" int nrsc5hip_fm_process(nrsc5hip_fm *f, const int16_t *dev_in, long long in_stride_elems, long long n_in, int16_t *dev_out,
                                   long long out_stride_elems, long long out_capacity, long long *n_out)
{
    if (!f) FAIL(NRSC5HIP_EINVAL, "null demodulator");
    long long nout = 0;
    int rc = nrsc5::fm_check_input(f, dev_in, in_stride_elems, n_in);
    if (rc) return rc;
    rc = nrsc5::fm_check(f, n_in, dev_out, out_stride_elems, out_capacity, &nout);
    if (rc) return rc;
    nrsc5::DeviceGuard guard(f->device);
    rc = nrsc5::fm_launch(f, f->stream, dev_in, in_stride_elems, n_in, dev_out, out_stride_elems);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(f->stream));               // outputs complete, dev_in no longer read
    if (n_out) *n_out = nout;
    return 0;
}

extern "C" int nrsc5hip_fm_debug_launches(nrsc5hip_fm *f, long long *count)
{
    if (!f || !count) FAIL(NRSC5HIP_EINVAL, "null argument");
    *count = f->launches;
    return 0;
}

extern "C" int nrsc5hip_fm_clip_counts(nrsc5hip_fm *f, long long *counts)
{
    if (!f || !counts) FAIL(NRSC5HIP_EINVAL, "null argument");
    nrsc5::DeviceGuard guard(f->device);
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpy(counts, f->d_clips, sizeof(long long) * 2 * f->nchan, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_fm_pilot(nrsc5hip_fm *f, float *level, int *stereo)
{
    if (!f || (!level && !stereo)) FAIL(NRSC5HIP_EINVAL, "null argument");
    nrsc5::DeviceGuard guard(f->device);
    HIPCHK(hipStreamSynchronize(f->stream));
    std::vector<float> v(2 * (size_t)f->nchan);
    HIPCHK(hipMemcpy(v.data(), f->d_pilot, sizeof(float) * v.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < f->nchan; k++) {
        if (level) level[k] = v[2 * k];
        if (stereo) stereo[k] = v[2 * k + 1] != 0.0f;
    }
    return 0;
}

extern "C" int nrsc5hip_stage_fm_mpx(nrsc5hip_fm *f, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *d_out, float *psum_out)
{
    if (!f || !d_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    nrsc5::DeviceGuard guard(f->device);
    StageFront sf;
    const int rc = sf.open(f, dev_in, in_stride_elems, n_in, false);
    if (rc) return rc;
    const long long m1 = sf.m1, b1 = sf.b1;
    nrsc5::DevTmp p;
    HIPCHK(hipMalloc(&p.p, sizeof(float2) * (size_t)(b1 + 1) * f->nchan));
    if (b1 > 0) {
        PilotArgs q;
        q.d = sf.df(); q.d_stride = m1; q.d_base = 0; q.cs = f->d_cs; q.p = (float2 *)p.p; q.p_stride = b1; q.p_base = 0; q.j0 = 0;
        launch_pilot(f->stream, (int)b1, f->nchan, q);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpy(d_out, sf.d.p, sizeof(float) * (size_t)m1 * f->nchan, hipMemcpyDeviceToHost));
    if (psum_out && b1 > 0) HIPCHK(hipMemcpy(psum_out, p.p, sizeof(float2) * (size_t)b1 * f->nchan, hipMemcpyDeviceToHost));
    return 0;
}

// ---- reception steering (include/nrsc5hip.h, "reception steering") ------------------------------------------------------------
namespace {

// a threshold in dB CNR as a value of q = (S / P)^2, in double
double steer_q_of_db(double db)
{
    const double rho = pow(10.0, db / 10.0), u = rho / (1.0 + rho);
    return u * u;
}

bool steer_ramp_of(const double db[2], float *lo, float *inv)
{
    if (!std::isfinite(db[0]) || !std::isfinite(db[1]) || !(db[1] > db[0])) return false;
    const double q_lo = steer_q_of_db(db[0]), q_hi = steer_q_of_db(db[1]);
    if (!(q_hi > q_lo)) return false;                        // (thresholds so high that both round to 1)
    *lo = (float)q_lo; *inv = (float)(1.0 / (q_hi - q_lo));
    return std::isfinite(*inv);
}

}  // namespace

extern "C" int nrsc5hip_fm_steer_enable(nrsc5hip_fm *f, const nrsc5hip_fm_steer_config *cfg)
{
    FM_ENABLE_CHECK(f, f->steer, "reception steering");
    nrsc5hip_fm_steer_config c = {NRSC5HIP_FM_STEER_ALL, {18.0, 30.0}, {10.0, 20.0}, {2.0, 8.0}, -20.0};
    if (cfg) c = *cfg;
    if (c.controls & ~(unsigned)NRSC5HIP_FM_STEER_ALL) FAIL(NRSC5HIP_EINVAL, "controls 0x%x: unknown bits", c.controls);
    SteerRamps r = {};
    r.controls = c.controls;
    if (!steer_ramp_of(c.blend_db, &r.blend_lo, &r.blend_inv)) FAIL(NRSC5HIP_EINVAL, "blend thresholds %g, %g dB: finite, the second above the first", c.blend_db[0], c.blend_db[1]);
    if (!steer_ramp_of(c.highcut_db, &r.highcut_lo, &r.highcut_inv))
        FAIL(NRSC5HIP_EINVAL, "high-cut thresholds %g, %g dB: finite, the second above the first", c.highcut_db[0], c.highcut_db[1]);
    if (!steer_ramp_of(c.mute_db, &r.mute_lo, &r.mute_inv)) FAIL(NRSC5HIP_EINVAL, "mute thresholds %g, %g dB: finite, the second above the first", c.mute_db[0], c.mute_db[1]);
    if (!std::isfinite(c.mute_floor_db) || c.mute_floor_db > 0.0) FAIL(NRSC5HIP_EINVAL, "mute_floor_db %g: finite, at most 0", c.mute_floor_db);
    r.mute_floor = (float)pow(10.0, c.mute_floor_db / 20.0);
    int tb = 0;
    std::vector<float> tab_n = audio_prototype(PASS_N, STOP_N, f->deemphasis_us, &tb);
    if (tb != f->tb) FAIL(NRSC5HIP_EINVAL, "the narrow table has %d taps per phase, the wide one %d", tb, f->tb);      // (the same transition width: never)
    const std::vector<float> dev = device_layout(tab_n, tb);
    nrsc5::DeviceGuard guard(f->device);
    nrsc5::DevTmp d_tab, d_steer;
    HIPCHK(hipMalloc(&d_tab.p, sizeof(float) * dev.size()));
    HIPCHK(hipMalloc(&d_steer.p, sizeof(float4) * f->nchan));
    HIPCHK(hipMemcpy(d_tab.p, dev.data(), sizeof(float) * dev.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_steer.p, 0, sizeof(float4) * f->nchan));
    if (!f->carrier) { const int rc = nrsc5::carrier_enable(f); if (rc) return rc; }
    f->d_tab_n = (float *)d_tab.p; f->d_steer = (float4 *)d_steer.p; d_tab.p = d_steer.p = nullptr;
    f->tab_n.swap(tab_n); f->ramps = r; f->steer = true;
    return 0;
}

extern "C" int nrsc5hip_fm_steer(nrsc5hip_fm *f, nrsc5hip_fm_steer_info *out)
{
    if (!f || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    FM_FEATURE_ENTER(f, steer, "reception steering");
    static_assert(sizeof(nrsc5hip_fm_steer_info) == sizeof(float4), "the device writes (q, b, h, g) as one float4");
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpy(out, f->d_steer, sizeof(float4) * f->nchan, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_fm_steer_taps(nrsc5hip_fm *f, float *audio_narrow)
{
    if (!f || !audio_narrow) FAIL(NRSC5HIP_EINVAL, "null argument");
    FM_FEATURE_ENTER(f, steer, "reception steering");
    memcpy(audio_narrow, f->tab_n.data(), sizeof(float) * f->tab_n.size());
    return 0;
}

extern "C" int nrsc5hip_stage_fm_steer(nrsc5hip_fm *f, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *out)
{
    if (!f || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    FM_FEATURE_ENTER(f, steer, "reception steering");
    StageFront sf;
    const int rc = sf.open(f, dev_in, in_stride_elems, n_in, true, W + 1);
    if (rc) return rc;
    const long long m1 = sf.m1, b1 = sf.b1, a1 = b1 > W ? b1 - W : 0;
    if (a1 == 0) return 0;                                   // no audio block
    const size_t K = (size_t)f->nchan;
    nrsc5::DevTmp p, t, pcm, fac, clips, pilot;
    HIPCHK(hipMalloc(&p.p, sizeof(float2) * (size_t)b1 * K));
    HIPCHK(hipMalloc(&t.p, sizeof(double) * 3 * (size_t)b1 * K));
    HIPCHK(hipMalloc(&pcm.p, sizeof(int16_t) * 2 * BLOCK_OUT * (size_t)a1 * K));
    HIPCHK(hipMalloc(&fac.p, sizeof(float4) * (size_t)a1 * K));
    HIPCHK(hipMalloc(&clips.p, sizeof(unsigned long long) * 2 * K));
    HIPCHK(hipMalloc(&pilot.p, sizeof(float) * 2 * K));
    HIPCHK(hipMemsetAsync(clips.p, 0, sizeof(unsigned long long) * 2 * K, f->stream));
    PilotArgs q;
    q.d = sf.df(); q.d_stride = m1; q.d_base = 0; q.cs = f->d_cs; q.p = (float2 *)p.p; q.p_stride = b1; q.p_base = 0; q.j0 = 0;
    launch_pilot(f->stream, (int)b1, f->nchan, q);
    HIPCHK(hipGetLastError());
    CarrierArgs c;
    c.r = sf.rf(); c.r_stride = m1; c.r_base = 0; c.d = sf.df(); c.d_stride = m1; c.d_base = 0;
    c.t = (double *)t.p; c.t_stride = b1; c.t_base = 0; c.j0 = 0;
    launch_carrier(f->stream, (int)b1, f->nchan, c);
    HIPCHK(hipGetLastError());
    SteeredAudioArgs u;
    u.d = sf.df(); u.d_stride = m1; u.d_base = 0; u.p = (const float2 *)p.p; u.p_stride = b1; u.p_base = 0; u.cs = f->d_cs;
    u.tab = f->d_tab; u.tb = f->tb; u.win = f->d_win; u.wsum = f->wsum; u.aq = f->aq; u.bq = f->bq; u.pilot_min = f->pilot_min; u.scale = f->d_scale;
    u.j0 = 0; u.k0 = 0; u.out = (int16_t *)pcm.p; u.out_stride = 2 * BLOCK_OUT * a1; u.clips = (unsigned long long *)clips.p; u.pilot = (float *)pilot.p;
    u.t = (const double *)t.p; u.t_stride = b1; u.t_base = 0; u.tab_n = f->d_tab_n; u.ramps = f->ramps;
    u.steer = (float4 *)fac.p; u.steer_stride = a1; u.steer_every = 1;
    launch_audio_steered(f->stream, (int)a1, f->nchan, u);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpy(out, fac.p, sizeof(float4) * (size_t)a1 * K, hipMemcpyDeviceToHost));
    return 0;
}
