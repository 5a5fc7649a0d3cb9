// Wideband channelizer (include/nrsc5hip.h, "wideband channelizer"): one complex capture at any rate Fs_in in [744 187.5, 64 M] S/s
// -> K reference-format cs16 streams at 744 187.5 S/s, each what a tuner centred at offset f_k would hand to nrsc5_pipe_samples_cs16.
//
// Per channel: integer-phase mixer (theta[n] = n * s_k mod 2^32, never drifts), then a polyphase resampler whose output m sits at
// input time t_m = m * P / Q (exact reduced fraction), split in 64-bit integers into floor(t_m) and the phase (m * P mod Q) / Q.  The
// lowpass prototype h (Kaiser-windowed sinc, designed on the host in double) is stored as a float32 table of L phases x T taps; an
// output uses the nearest phase.  The arithmetic of one output (its phase row, the input samples it reads, the order of its sum) depends
// only on absolute sample indices, so any chunking of the input gives the same bytes.
//
// Kernel: one workgroup = one tile of `mt` consecutive outputs (aligned to absolute output indices) x one group of GROUP channels.  The
// input span of the tile is read once per channel group (later channels hit L2), mixed per channel into LDS (one sincos per input
// sample and channel), and every work-item sums one output's T taps for CG channels at a time, so that each table load feeds
// 2 * CG FMAs (I and Q packed: v_pk_fma_f32).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <string>
#include <vector>
#include "nrsc5hip.h"
#include "host_util.h"
#include "fm_audio.h"

namespace {

constexpr long long OUT_RATE_NUM = 1488375, OUT_RATE_DEN = 2;   // 744 187.5 S/s: the one place the output rate lives
constexpr double PASS_HZ = 198.5e3;                              // outermost FM carrier, bin 546 x 363.4 Hz = 198.4 kHz
constexpr double STOP_HZ = 545.8e3;                              // 744 187.5 - 198.4 k: lowest frequency that aliases into the sidebands
constexpr double DESIGN_ATTEN_DB = 80.0;                         // Kaiser design target (the contract is 70 dB)
constexpr double PHASE_RATE = 3.5e9;                             // L = PHASE_RATE / Fs_in: nearest-phase timing error ~ -84 dB of the signal
constexpr int MAX_CHANNELS = 512;
constexpr int CG = 2;                                            // channels per pass of the FIR loop (one table load -> 2 * CG FMAs)
constexpr int SPAN_MAX = 4096;                                   // input samples of one tile; LDS = CG * SPAN_MAX * 8 = 64 KiB
constexpr int GROUP = 8;                                         // channels per workgroup (grid.y = ceil(K / GROUP))

struct ChanArgs {
    const void *in; int fmt; int T; long long n0, n_in;     // new input = absolute samples [n0, n0 + n_in)
    const float2 *hist;                                     // absolute samples [n0 - T, n0), scaled (zeros before n = 0)
    const float *table; const unsigned *step; const float *gain;
    unsigned long long P, Q; int L, mt, span, nchan;
    long long m_a, i_a, n_out; unsigned long long r_a;      // outputs [m_a, m_a + n_out); m_a * P = i_a * Q + r_a
    int16_t *out; long long stride; unsigned long long *clips;
};

__device__ __forceinline__ float2 load_new(const void *in, int fmt, long long k)
{
    if (fmt == NRSC5HIP_IQ_CU8) {
        const uint8_t *p = (const uint8_t *)in + 2 * k;
        return make_float2((float)(((int)p[0] - 127) * 64), (float)(((int)p[1] - 127) * 64));   // U8_Q15, defines.h:93
    }
    if (fmt == NRSC5HIP_IQ_CS16) {
        const int16_t *p = (const int16_t *)in + 2 * k;
        return make_float2((float)p[0], (float)p[1]);
    }
    const float *p = (const float *)in + 2 * k;
    return make_float2(p[0] * 32768.0f, p[1] * 32768.0f);
}

// scaled sample at absolute index n; samples not yet pushed read as 0 (only the zero last tap of a phase rounded up to the next
// input sample can reach one)
__device__ __forceinline__ float2 load_sample(const ChanArgs &a, long long n)
{
    if (n >= a.n0) return n < a.n0 + a.n_in ? load_new(a.in, a.fmt, n - a.n0) : make_float2(0.0f, 0.0f);
    const long long h = n - (a.n0 - a.T);
    return h >= 0 ? a.hist[h] : make_float2(0.0f, 0.0f);
}

// output m_a + d -> anchor i (floor(t_m), or floor(t_m) + 1 when the phase rounds up to a whole sample) and nearest phase row p
__device__ __forceinline__ void out_pos(const ChanArgs &a, long long d, long long *i, int *p)
{
    const unsigned long long q = (unsigned long long)d * a.P + a.r_a;
    long long ii = a.i_a + (long long)(q / a.Q);
    const unsigned long long r = q % a.Q;
    unsigned long long pp = (r * (unsigned long long)a.L + a.Q / 2) / a.Q;
    if (pp == (unsigned long long)a.L) { ii += 1; pp = 0; }
    *i = ii; *p = (int)pp;
}

__global__ __launch_bounds__(256) void k_channelize(ChanArgs a)
{
    HIP_DYNAMIC_SHARED(float2, mixed);                       // [CG][span]
    const long long tile0 = (a.m_a / a.mt + (long long)blockIdx.x) * a.mt;
    long long d_first = tile0 - a.m_a, d_end = tile0 + a.mt - a.m_a;
    if (d_first < 0) d_first = 0;
    if (d_end > a.n_out) d_end = a.n_out;
    if (d_first >= d_end) return;
    long long i_first, i_last; int p_unused;
    out_pos(a, d_first, &i_first, &p_unused);
    out_pos(a, d_end - 1, &i_last, &p_unused);
    const int half = a.T / 2;
    const long long n_lo = i_first - half + 1;
    int span = (int)(i_last + half - n_lo + 1);
    if (span > a.span) span = a.span;                        // the host's bound: never reached

    const long long d = tile0 - a.m_a + threadIdx.x;
    const bool valid = (int)threadIdx.x < a.mt && d >= d_first && d < d_end;
    long long i = i_first; int p = 0;
    if (valid) out_pos(a, d, &i, &p);
    const float *h = a.table + (size_t)p * a.T;
    const int off = (int)(i - half + 1 - n_lo);

    const int c_begin = blockIdx.y * GROUP, c_end = min(a.nchan, c_begin + GROUP);
    for (int c0 = c_begin; c0 < c_end; c0 += CG) {
        const int nc = min(CG, c_end - c0);
        __syncthreads();                                     // the previous pass is done with mixed[]
        for (int k = threadIdx.x; k < span; k += blockDim.x) {
            const long long n = n_lo + k;
            const float2 x = load_sample(a, n);
            for (int c = 0; c < nc; c++) {
                const unsigned th = (unsigned)(unsigned long long)n * a.step[c0 + c];     // exact phase, mod 2^32
                const float rev = (float)(int)th * 2.3283064365386963e-10f;            // revolutions in [-0.5, 0.5)
                float sn, cs;
                __sincosf(6.283185307179586f * rev, &sn, &cs);
                mixed[c * a.span + k] = make_float2(x.x * cs + x.y * sn, x.y * cs - x.x * sn);   // x * exp(-j theta)
            }
        }
        __syncthreads();
        if (!valid) continue;
        float re[CG], im[CG];
        for (int c = 0; c < CG; c++) { re[c] = 0.0f; im[c] = 0.0f; }
        if (nc == CG) {
            const float2 *v0 = mixed + off, *v1 = mixed + a.span + off;
            for (int j = 0; j < a.T; j++) {
                const float t = h[j];
                const float2 x0 = v0[j], x1 = v1[j];
                re[0] = fmaf(x0.x, t, re[0]); im[0] = fmaf(x0.y, t, im[0]);
                re[1] = fmaf(x1.x, t, re[1]); im[1] = fmaf(x1.y, t, im[1]);
            }
        } else {
            const float2 *v0 = mixed + off;
            for (int j = 0; j < a.T; j++) {
                const float t = h[j];
                const float2 x0 = v0[j];
                re[0] = fmaf(x0.x, t, re[0]); im[0] = fmaf(x0.y, t, im[0]);
            }
        }
        for (int c = 0; c < nc; c++) {
            const int ch = c0 + c;
            const float g = a.gain[ch];
            float yr = rintf(re[c] * g), yi = rintf(im[c] * g);
            int clipped = 0;
            if (yr > 32767.0f) { yr = 32767.0f; clipped = 1; } else if (yr < -32768.0f) { yr = -32768.0f; clipped = 1; }
            if (yi > 32767.0f) { yi = 32767.0f; clipped = 1; } else if (yi < -32768.0f) { yi = -32768.0f; clipped = 1; }
            if (clipped) atomicAdd(a.clips + ch, 1ull);
            int16_t *o = a.out + ch * a.stride + 2 * d;
            o[0] = (int16_t)(int)yr;
            o[1] = (int16_t)(int)yi;
        }
    }
}

// history for the next call: absolute samples [n1 - T, n1), n1 = n0 + n_in
__global__ __launch_bounds__(256) void k_chan_history(const void *in, int fmt, long long n0, long long n_in, const float2 *hist_old,
                                                      float2 *hist_new, int T)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= T) return;
    const long long n = n0 + n_in - T + k;
    float2 v;
    if (n >= n0) v = load_new(in, fmt, n - n0);
    else v = hist_old[n - (n0 - T)];                        // n >= n0 - T: the old history holds it
    hist_new[k] = v;
}

double bessel_i0(double x)
{
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 500; k++) {
        t *= (x / (2.0 * k)) * (x / (2.0 * k));
        s += t;
        if (t < 1e-18 * s) break;
    }
    return s;
}

unsigned long long gcd_u64(unsigned long long a, unsigned long long b) { while (b) { unsigned long long t = a % b; a = b; b = t; } return a; }

}  // namespace

struct nrsc5hip_chan {
    int device = 0, fmt = 0, nchan = 0;
    double fs = 0;
    unsigned long long P = 1, Q = 1;
    int T = 0, L = 0, mt = 0, span = 0;
    std::vector<unsigned> step;
    std::vector<float> gain;
    std::vector<float> table;                               // host copy, [L][T]
    hipStream_t stream = nullptr;
    hipEvent_t ev_out = nullptr, ev_eng = nullptr;
    bool eng_pending = false;                               // ev_eng: the engine's last append from d_feed
    float *d_table = nullptr, *d_gain = nullptr;
    unsigned *d_step = nullptr;
    float2 *d_hist[2] = {nullptr, nullptr};
    int cur = 0;
    unsigned long long *d_clips = nullptr, *d_clips_saved = nullptr;   // _feed restores the counts when the engine refuses an append
    int16_t *d_feed = nullptr; long long feed_cap = 0;      // _feed's staging: outputs per channel it holds
    long long n_total = 0, m_total = 0;                     // input samples pushed / outputs produced since create or reset
};

namespace {
// number of outputs m with floor(t_m) + T/2 < n, i.e. m >= 0 with floor(m P / Q) <= n - 1 - T/2
long long outputs_total(const nrsc5hip_chan *c, long long n)
{
    const long long a1 = n - c->T / 2;
    if (a1 <= 0) return 0;
    const unsigned __int128 num = (unsigned __int128)(unsigned long long)a1 * c->Q + (c->P - 1);
    return (long long)(num / c->P);
}

void free_chan(nrsc5hip_chan *c)
{
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->eng_pending) (void)hipEventSynchronize(c->ev_eng);
    (void)hipFree(c->d_table); (void)hipFree(c->d_gain); (void)hipFree(c->d_step);
    (void)hipFree(c->d_hist[0]); (void)hipFree(c->d_hist[1]); (void)hipFree(c->d_clips); (void)hipFree(c->d_clips_saved); (void)hipFree(c->d_feed);
    if (c->ev_out) (void)hipEventDestroy(c->ev_out);
    if (c->ev_eng) (void)hipEventDestroy(c->ev_eng);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int chan_zero_state(nrsc5hip_chan *c)
{
    if (c->eng_pending) { HIPCHK(hipEventSynchronize(c->ev_eng)); c->eng_pending = false; }
    HIPCHK(hipMemsetAsync(c->d_hist[0], 0, sizeof(float2) * c->T, c->stream));
    HIPCHK(hipMemsetAsync(c->d_hist[1], 0, sizeof(float2) * c->T, c->stream));
    HIPCHK(hipMemsetAsync(c->d_clips, 0, sizeof(unsigned long long) * c->nchan, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->cur = 0; c->n_total = 0; c->m_total = 0;
    return 0;
}

// FIR + history update on the channelizer's stream; outputs [m_total, m_total + nout) go to out + k * stride.  No host wait.
int chan_launch(nrsc5hip_chan *c, const void *dev_in, long long n_in, long long nout, int16_t *out, long long stride)
{
    if (n_in <= 0) return 0;
    if (nout > 0) {
        const long long tiles = (c->m_total + nout - 1) / c->mt - c->m_total / c->mt + 1;
        if (tiles > 0x7fffffffLL) FAIL(NRSC5HIP_EINVAL, "push too large: %lld output tiles", tiles);
        ChanArgs a;
        a.in = dev_in; a.fmt = c->fmt; a.T = c->T; a.n0 = c->n_total; a.n_in = n_in; a.hist = c->d_hist[c->cur];
        a.table = c->d_table; a.step = c->d_step; a.gain = c->d_gain; a.P = c->P; a.Q = c->Q; a.L = c->L; a.mt = c->mt;
        a.span = c->span; a.nchan = c->nchan; a.m_a = c->m_total; a.n_out = nout; a.out = out; a.stride = stride; a.clips = c->d_clips;
        const unsigned __int128 mp = (unsigned __int128)(unsigned long long)c->m_total * c->P;
        a.i_a = (long long)(mp / c->Q); a.r_a = (unsigned long long)(mp % c->Q);
        const int block = c->mt < 64 ? 64 : c->mt;
        dim3 grid((unsigned)tiles, (unsigned)((c->nchan + GROUP - 1) / GROUP));
        hipLaunchKernelGGL(k_channelize, grid, dim3(block), (size_t)CG * c->span * sizeof(float2), c->stream, a);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_chan_history, dim3((c->T + 255) / 256), dim3(256), 0, c->stream, dev_in, c->fmt, c->n_total, n_in,
                       (const float2 *)c->d_hist[c->cur], c->d_hist[c->cur ^ 1], c->T);
    HIPCHK(hipGetLastError());
    c->cur ^= 1;
    c->n_total += n_in;
    c->m_total += nout;
    return 0;
}
}  // namespace

extern "C" int nrsc5hip_chan_create(const nrsc5hip_chan_config *cfg, nrsc5hip_chan **out)
{
    if (!cfg || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->format < NRSC5HIP_IQ_CU8 || cfg->format > NRSC5HIP_IQ_CF32) FAIL(NRSC5HIP_EINVAL, "bad input format %d", cfg->format);
    if (cfg->nchan < 1 || cfg->nchan > MAX_CHANNELS) FAIL(NRSC5HIP_EINVAL, "nchan %d out of range 1..%d", cfg->nchan, MAX_CHANNELS);
    if (!cfg->offset_hz) FAIL(NRSC5HIP_EINVAL, "null offset_hz");
    if (cfg->rate_num <= 0 || cfg->rate_den <= 0) FAIL(NRSC5HIP_EINVAL, "rate %lld/%lld not positive", cfg->rate_num, cfg->rate_den);
    const __int128 num = cfg->rate_num, den = cfg->rate_den;          // 744 187.5 <= num / den <= 64e6, exactly
    if (num * OUT_RATE_DEN < (__int128)OUT_RATE_NUM * den || num > (__int128)64000000 * den)
        FAIL(NRSC5HIP_EINVAL, "rate %lld/%lld S/s outside 744187.5 .. 64e6", cfg->rate_num, cfg->rate_den);
    // R = Fs_in / 744 187.5 = (num * 2) / (den * 1488375) = P / Q, reduced
    const __int128 p128 = num * OUT_RATE_DEN, q128 = den * OUT_RATE_NUM;
    if (p128 >= ((__int128)1 << 62) || q128 >= ((__int128)1 << 62)) FAIL(NRSC5HIP_EINVAL, "rate %lld/%lld: terms too large", cfg->rate_num, cfg->rate_den);
    unsigned long long P = (unsigned long long)p128, Q = (unsigned long long)q128;
    const unsigned long long g = gcd_u64(P, Q);
    P /= g; Q /= g;
    if (P >= (1ull << 31) || Q >= (1ull << 31))
        FAIL(NRSC5HIP_EINVAL, "rate %lld/%lld: resampling ratio %llu/%llu needs terms below 2^31", cfg->rate_num, cfg->rate_den, P, Q);
    const double fs = (double)cfg->rate_num / (double)cfg->rate_den;
    for (int k = 0; k < cfg->nchan; k++) {
        const double f = cfg->offset_hz[k];
        if (!(fabs(f) <= fs / 2 - PASS_HZ)) FAIL(NRSC5HIP_EINVAL, "channel %d: |offset| %.1f Hz > Fs/2 - %.1f Hz", k, f, PASS_HZ);
        if (cfg->gain && !std::isfinite(cfg->gain[k])) FAIL(NRSC5HIP_EINVAL, "channel %d: gain not finite", k);
    }
    // prototype: Kaiser-windowed sinc, cut-off half-way through the transition band, support T input samples
    const double beta = 0.1102 * (DESIGN_ATTEN_DB - 8.7);
    const double dw = 2.0 * M_PI * (STOP_HZ - PASS_HZ) / fs;
    int T = (int)ceil((DESIGN_ATTEN_DB - 7.95) / (2.285 * dw)) + 1;
    T += T & 1;
    if (T < 8) T = 8;
    int L = (int)ceil(PHASE_RATE / fs);
    L = L < 32 ? 32 : L > 4096 ? 4096 : L;
    // tile: the largest power of two (16..256) of outputs whose input span fits SPAN_MAX.  Both terms of the span grow with the rate, and
    // at the 64 MS/s cap a tile of 32 spans 31 * 86 + 926 + 2 = 3593 samples: the loop never gets to its floor of 16, which no test can
    // therefore reach (tests/chan_model.py: RATE_EDGE_CASES runs 256, 64 and 32).  The floor stays as the loop's end, not as a case.
    int mt = 256;
    for (; mt > 16; mt /= 2)
        if ((long long)((mt - 1) * (unsigned __int128)P / Q) + T + 2 <= SPAN_MAX) break;
    const long long span = (long long)((mt - 1) * (unsigned __int128)P / Q) + T + 2;
    if (span > SPAN_MAX) FAIL(NRSC5HIP_EINVAL, "rate %lld/%lld: tile span %lld exceeds %d", cfg->rate_num, cfg->rate_den, span, SPAN_MAX);

    nrsc5hip_chan *c = new (std::nothrow) nrsc5hip_chan;
    if (!c) FAIL(NRSC5HIP_ENOMEM, "out of host memory");
    c->device = cfg->device; c->fmt = cfg->format; c->nchan = cfg->nchan;
    c->fs = fs; c->P = P; c->Q = Q; c->T = T; c->L = L; c->mt = mt; c->span = (int)span;
    for (int k = 0; k < cfg->nchan; k++) {
        const long long s = llround(cfg->offset_hz[k] / fs * 4294967296.0);
        c->step.push_back((unsigned)(unsigned long long)s);
        c->gain.push_back(cfg->gain ? cfg->gain[k] : 1.0f);
    }
    const double fc = 0.5 * (PASS_HZ + STOP_HZ) / fs, i0b = bessel_i0(beta);
    c->table.resize((size_t)L * T);
    for (int p = 0; p < L; p++)
        for (int j = 0; j < T; j++) {
            const double tau = (double)p / L + T / 2 - 1 - j, u = 2.0 * tau / T;   // h(t_m - n), n = floor(t_m) - T/2 + 1 + j
            double v = 0.0;
            if (fabs(u) < 1.0) {
                const double x = 2.0 * fc * tau;
                const double sinc = x == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x);
                v = 2.0 * fc * sinc * bessel_i0(beta * sqrt(1.0 - u * u)) / i0b;
            }
            c->table[(size_t)p * T + j] = (float)v;
        }

    nrsc5::DeviceGuard guard(c->device);
#define CREATE_CHK(expr) HIPCHK_OR(expr, free_chan(c))
    CREATE_CHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CREATE_CHK(hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
    CREATE_CHK(hipEventCreateWithFlags(&c->ev_eng, hipEventDisableTiming));
    CREATE_CHK(hipMalloc(&c->d_table, sizeof(float) * c->table.size()));
    CREATE_CHK(hipMalloc(&c->d_gain, sizeof(float) * c->nchan));
    CREATE_CHK(hipMalloc(&c->d_step, sizeof(unsigned) * c->nchan));
    CREATE_CHK(hipMalloc(&c->d_hist[0], sizeof(float2) * T));
    CREATE_CHK(hipMalloc(&c->d_hist[1], sizeof(float2) * T));
    CREATE_CHK(hipMalloc(&c->d_clips, sizeof(unsigned long long) * c->nchan));
    CREATE_CHK(hipMalloc(&c->d_clips_saved, sizeof(unsigned long long) * c->nchan));
    CREATE_CHK(hipMemcpy(c->d_table, c->table.data(), sizeof(float) * c->table.size(), hipMemcpyHostToDevice));
    CREATE_CHK(hipMemcpy(c->d_gain, c->gain.data(), sizeof(float) * c->nchan, hipMemcpyHostToDevice));
    CREATE_CHK(hipMemcpy(c->d_step, c->step.data(), sizeof(unsigned) * c->nchan, hipMemcpyHostToDevice));
#undef CREATE_CHK
    int rc = chan_zero_state(c);
    if (rc) { free_chan(c); return rc; }
    *out = c;
    return 0;
}

extern "C" void nrsc5hip_chan_destroy(nrsc5hip_chan *c)
{
    if (!c) return;
    nrsc5::DeviceGuard guard(c->device);
    free_chan(c);
}

extern "C" int nrsc5hip_chan_reset(nrsc5hip_chan *c)
{
    if (!c) FAIL(NRSC5HIP_EINVAL, "null channelizer");
    nrsc5::DeviceGuard guard(c->device);
    HIPCHK(hipStreamSynchronize(c->stream));
    return chan_zero_state(c);
}

extern "C" int nrsc5hip_chan_info(nrsc5hip_chan *c, double *realised_offset_hz, int *taps, int *phases)
{
    if (!c) FAIL(NRSC5HIP_EINVAL, "null channelizer");
    if (realised_offset_hz)
        for (int k = 0; k < c->nchan; k++) realised_offset_hz[k] = (double)(int)c->step[k] * c->fs / 4294967296.0;
    if (taps) *taps = c->T;
    if (phases) *phases = c->L;
    return 0;
}

extern "C" int nrsc5hip_chan_taps(nrsc5hip_chan *c, float *table)
{
    if (!c || !table) FAIL(NRSC5HIP_EINVAL, "null argument");
    memcpy(table, c->table.data(), sizeof(float) * c->table.size());
    return 0;
}

extern "C" long long nrsc5hip_chan_outputs_for(nrsc5hip_chan *c, long long n_in)
{
    if (!c) FAIL(NRSC5HIP_EINVAL, "null channelizer");
    if (n_in < 0) FAIL(NRSC5HIP_EINVAL, "n_in %lld negative", n_in);
    return outputs_total(c, c->n_total + n_in) - c->m_total;
}

extern "C" int nrsc5hip_chan_process(nrsc5hip_chan *c, const void *dev_in, long long n_in, int16_t *dev_out, long long out_stride_elems,
                                     long long out_capacity, long long *n_out)
{
    if (!c) FAIL(NRSC5HIP_EINVAL, "null channelizer");
    if (n_in < 0 || (n_in > 0 && !dev_in)) FAIL(NRSC5HIP_EINVAL, "bad input (n_in %lld)", n_in);
    const long long nout = outputs_total(c, c->n_total + n_in) - c->m_total;
    if (nout > 0 && !dev_out) FAIL(NRSC5HIP_EINVAL, "null output");
    if (out_capacity < 0 || (c->nchan > 1 && out_stride_elems < 2 * out_capacity))
        FAIL(NRSC5HIP_EINVAL, "out_stride_elems %lld < 2 * out_capacity %lld", out_stride_elems, out_capacity);
    if (nout > out_capacity) FAIL(NRSC5HIP_EOVERFLOW, "push of %lld samples yields %lld outputs per channel > out_capacity %lld", n_in, nout, out_capacity);
    nrsc5::DeviceGuard guard(c->device);
    int rc = chan_launch(c, dev_in, n_in, nout, dev_out, out_stride_elems);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));               // outputs complete, dev_in no longer read
    if (n_out) *n_out = nout;
    return 0;
}

extern "C" int nrsc5hip_chan_clip_counts(nrsc5hip_chan *c, long long *counts)
{
    if (!c || !counts) FAIL(NRSC5HIP_EINVAL, "null argument");
    nrsc5::DeviceGuard guard(c->device);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(counts, c->d_clips, sizeof(long long) * c->nchan, hipMemcpyDeviceToHost));
    return 0;
}

namespace {
// nrsc5hip_chan_feed; with fm, the demodulator then reads the staged outputs on the channelizer's stream, in front of the next push's write
int chan_feed_impl(nrsc5hip_chan *c, nrsc5hip_engine *e, const int *stream_ids, const void *dev_in, long long n_in, nrsc5hip_fm *fm,
                   int16_t *dev_audio, long long audio_stride, long long audio_capacity, long long *n_audio)
{
    if (!c || !e || !stream_ids) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (n_in < 0 || (n_in > 0 && !dev_in)) FAIL(NRSC5HIP_EINVAL, "bad input (n_in %lld)", n_in);
    const long long nout = outputs_total(c, c->n_total + n_in) - c->m_total;
    if (2 * nout > 0xffffffffLL) FAIL(NRSC5HIP_EINVAL, "push too large for one append (%lld outputs)", nout);
    if (fm) {
        if (nrsc5::fm_nchan(fm) != c->nchan || nrsc5::fm_device(fm) != c->device)
            FAIL(NRSC5HIP_EINVAL, "demodulator has %d channels on device %d, the channelizer %d on device %d", nrsc5::fm_nchan(fm), nrsc5::fm_device(fm), c->nchan, c->device);
        int rc = nrsc5::fm_check(fm, nout, dev_audio, audio_stride, audio_capacity, n_audio);   // (the staging buffer: 4-byte aligned, even stride)
        if (rc) return rc;
    }
    nrsc5::DeviceGuard guard(c->device);
    if (nout > c->feed_cap) {                               // grow the staging buffer once the engine has read the old one
        if (c->eng_pending) { HIPCHK(hipEventSynchronize(c->ev_eng)); c->eng_pending = false; }
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(c->d_feed)); c->d_feed = nullptr; c->feed_cap = 0;
        const long long cap = nout + nout / 4 + 1024;
        HIPCHK(hipMalloc(&c->d_feed, sizeof(int16_t) * 2 * (size_t)cap * c->nchan));
        c->feed_cap = cap;
    }
    if (c->eng_pending) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_eng, 0));   // the engine's previous append has read the buffer
    // the state before this push: an append the engine refuses (stream id, q15_capacity) leaves the channelizer as it was
    const int cur0 = c->cur; const long long n0 = c->n_total, m0 = c->m_total;
    HIPCHK(hipMemcpyAsync(c->d_clips_saved, c->d_clips, sizeof(unsigned long long) * c->nchan, hipMemcpyDeviceToDevice, c->stream));
    int rc = chan_launch(c, dev_in, n_in, nout, c->d_feed, 2 * c->feed_cap);
    if (rc) return rc;
    if (nout > 0) {
        hipStream_t es = (hipStream_t)nrsc5hip_engine_hip_stream(e);
        HIPCHK(hipEventRecord(c->ev_out, c->stream));
        HIPCHK(hipStreamWaitEvent(es, c->ev_out, 0));
        std::vector<uint32_t> nelems(c->nchan, (uint32_t)(2 * nout));
        rc = nrsc5hip_batch_append_cs16(e, c->nchan, stream_ids, c->d_feed, 2 * c->feed_cap, nelems.data());
        if (rc) {
            std::string msg = nrsc5hip_last_error();
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipMemcpy(c->d_clips, c->d_clips_saved, sizeof(unsigned long long) * c->nchan, hipMemcpyDeviceToDevice));
            c->cur = cur0; c->n_total = n0; c->m_total = m0;        // the old history buffer was only read
            nrsc5::set_last_error(msg.c_str());
            return rc;
        }
        HIPCHK(hipEventRecord(c->ev_eng, es));
        c->eng_pending = true;
        if (fm) {
            rc = nrsc5::fm_launch(fm, c->stream, c->d_feed, 2 * c->feed_cap, nout, dev_audio, audio_stride);
            if (rc) return rc;
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));               // dev_in no longer read when the call returns
    return 0;
}
}  // namespace

extern "C" int nrsc5hip_chan_feed(nrsc5hip_chan *c, nrsc5hip_engine *e, const int *stream_ids, const void *dev_in, long long n_in)
{
    return chan_feed_impl(c, e, stream_ids, dev_in, n_in, nullptr, nullptr, 0, 0, nullptr);
}

extern "C" int nrsc5hip_chan_feed_fm(nrsc5hip_chan *c, nrsc5hip_engine *e, const int *stream_ids, nrsc5hip_fm *fm, const void *dev_in, long long n_in,
                                     int16_t *dev_audio, long long audio_stride_elems, long long audio_capacity, long long *n_audio)
{
    if (!fm) FAIL(NRSC5HIP_EINVAL, "null demodulator");
    return chan_feed_impl(c, e, stream_ids, dev_in, n_in, fm, dev_audio, audio_stride_elems, audio_capacity, n_audio);
}
