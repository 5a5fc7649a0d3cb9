// Band scan (include/nrsc5hip.h, "band scan"): an averaged power spectrum of one complex capture at any rate Fs in [744 187.5, 64 M] S/s
// (Welch: periodic Hann, nfft = 2^M in 512..8192, 50 % overlap, segments tied to absolute sample indices), and a host detector that
// finds the hybrid-FM signature in it: two flat digital sidebands at 129.4 .. 198.4 kHz on each side of a centre.
//
// Kernel: one workgroup of 256 work-items transforms whole segments in LDS, a run of consecutive segments per workgroup.  Per segment:
// coalesced loads of the capture with the format conversion and the window fused in, an in-place decimation-in-frequency FFT (a radix-2
// pass when M is odd, then radix-4 passes whose outputs are stored in the order 0, 2, 1, 3 so that LDS position p ends up holding
// X[bitrev_M(p)] -- the order is undone once, on the host, when the spectrum is read), and |X|^2 added into registers: work-item t owns
// positions t + 256 i.  After its run the workgroup writes ONE row of partial sums; k_scan_reduce adds the rows in row order, in
// double, into the running sum.  No float atomics: the same pushes give the same bytes.
//
// Overlap: segment s + 1 re-reads the second half of segment s.  That second read comes from L2, not from LDS: the same workgroup asks
// for the same lines a few microseconds after it first touched them (4 B per sample, run * nfft / 2 * 4 B <= 1 MiB per workgroup), and
// keeping the raw half in LDS instead would cost another 32 KiB at nfft 8192, which the 160 KiB of a CU do not have next to the
// transform's 136 KiB.  HBM traffic is (run + 1) / run of the capture at worst.
//
// Precision: the transform, the window and every sum are double.  A float32 transform was measured first, on the twin, against the
// float64 model with a tone 40 dB above the noise: its largest relative error in the noise bins was 3e-5 at nfft 512, 7.5e-5 at 2048
// and 1.4e-4 at 8192 -- at and over the 1e-4 the spectrum is held to (the rounding of the tone's large partial sums lands in the small
// bins).  FP64 vector arithmetic runs at half the FP32 rate on this part; what the kernel waits for is the barrier after every pass
// with one wave per SIMD, not VALU.
//
// LDS: nfft elements of 16 B (ds_read_b128: 64 banks of 4 B per 16-lane group) plus one element of padding after every 16, which keeps
// the passes with a butterfly span of 1 and of >= 16 elements conflict-free; 136 KiB at nfft 8192, one workgroup per CU there.
//
// Detector (nrsc5hip_scan_detect_psd, host, double, no device): see the comment at detect_psd below.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>
#include "nrsc5hip.h"
#include "host_util.h"

namespace {

constexpr long long MIN_RATE_NUM = 1488375, MIN_RATE_DEN = 2;    // 744 187.5 S/s, the channelizer's lower bound
constexpr int MIN_LOG2 = 9, MAX_LOG2 = 13;                        // nfft 512 .. 8192
constexpr int WG = 256;
constexpr int RUN_MAX = 64;                                       // segments summed in registers before one row is written
constexpr int ROWS_TARGET = 1024;                                 // workgroups of one push, while the runs stay below RUN_MAX
constexpr double CARRIER_HZ = 1488375.0 / 4096.0;                 // 363.373 Hz
constexpr double SB_LO_HZ = 356 * CARRIER_HZ, SB_HI_HZ = 546 * CARRIER_HZ;   // digital sidebands: carriers 356 .. 546 (PASS_HZ of k_channelize.hip)
constexpr double EDGE_HZ = 198.5e3;                               // a centre needs |c| <= Fs/2 - EDGE_HZ, as a channel of the channelizer does
constexpr double FLOOR_QUANTILE = 0.2;

struct __attribute__((aligned(16))) cplx { double x, y; };

struct ScanArgs {
    const void *in; int fmt; long long n0, n_in;              // new input = absolute samples [n0, n0 + n_in)
    const float2 *hist;                                        // absolute samples [n0 - (nfft - 1), n0), scaled
    const cplx *tw;                                            // exp(-2 pi i k / nfft), k < nfft
    const double *win;                                          // periodic Hann
    long long seg0; int nseg, run;                             // segments [seg0, seg0 + nseg), `run` of them per workgroup
    double *part;                                              // [gridDim.x][nfft] partial sums, bit-reversed positions
};

__device__ __forceinline__ float2 scan_load_new(const void *in, int fmt, long long k)
{
    if (fmt == NRSC5HIP_IQ_CU8) {
        const uint8_t *p = (const uint8_t *)in + 2 * k;
        return make_float2((float)(((int)p[0] - 127) * 64), (float)(((int)p[1] - 127) * 64));
    }
    if (fmt == NRSC5HIP_IQ_CS16) {
        const int16_t *p = (const int16_t *)in + 2 * k;
        return make_float2((float)p[0], (float)p[1]);
    }
    const float *p = (const float *)in + 2 * k;
    return make_float2(p[0] * 32768.0f, p[1] * 32768.0f);
}

__device__ __forceinline__ int lds_pos(int p) { return p + (p >> 4); }
__device__ __forceinline__ cplx mk(double x, double y) { cplx c; c.x = x; c.y = y; return c; }
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return mk(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return mk(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

template <int M>
__global__ __launch_bounds__(WG) void k_scan_psd(ScanArgs a)
{
    constexpr int N = 1 << M, NPT = N / WG, H = N / 2;
    HIP_DYNAMIC_SHARED(cplx, x);                             // [N + N / 16]
    const int tid = threadIdx.x;
    const int s_first = blockIdx.x * a.run, s_end = min(a.nseg, s_first + a.run);
    const long long hist0 = a.n0 - (N - 1);
    double acc[NPT];
#pragma unroll
    for (int i = 0; i < NPT; i++) acc[i] = 0.0;

    for (int s = s_first; s < s_end; s++) {
        const long long base = (a.seg0 + s) * H;
        __syncthreads();                                     // the previous segment's |X|^2 has been read
#pragma unroll
        for (int i = 0; i < NPT; i++) {
            const int j = tid + WG * i;
            const long long n = base + j;                    // n >= n0 - (N - 1): the segment was not complete before this push
            const float2 v = n >= a.n0 ? scan_load_new(a.in, a.fmt, n - a.n0) : a.hist[n - hist0];
            const double w = a.win[j];
            x[lds_pos(j)] = mk((double)v.x * w, (double)v.y * w);
        }
        __syncthreads();
        int span = N;
        if (M & 1) {
            for (int b = tid; b < H; b += WG) {
                const cplx u = x[lds_pos(b)], v = x[lds_pos(b + H)];
                x[lds_pos(b)] = cadd(u, v);
                x[lds_pos(b + H)] = cmul(csub(u, v), a.tw[b]);
            }
            __syncthreads();
            span = H;
        }
        for (; span >= 4; span >>= 2) {
            const int q = span >> 2, tstep = N / span;
            for (int b = tid; b < N / 4; b += WG) {
                const int j = b & (q - 1), p0 = (b - j) * 4 + j;
                const int i0 = lds_pos(p0), i1 = lds_pos(p0 + q), i2 = lds_pos(p0 + 2 * q), i3 = lds_pos(p0 + 3 * q);
                const cplx a0 = x[i0], a1 = x[i1], a2 = x[i2], a3 = x[i3];
                const cplx t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = csub(a1, a3);
                const cplx mi = mk(t3.y, -t3.x);                                  // -i t3
                x[i0] = cadd(t0, t2);                                              // frequencies 4k
                x[i1] = cmul(csub(t0, t2), a.tw[2 * j * tstep]);                   // 4k + 2
                x[i2] = cmul(cadd(t1, mi), a.tw[j * tstep]);                       // 4k + 1
                x[i3] = cmul(csub(t1, mi), a.tw[3 * j * tstep]);                   // 4k + 3
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < NPT; i++) {
            const cplx v = x[lds_pos(tid + WG * i)];
            acc[i] += v.x * v.x + v.y * v.y;
        }
    }
    double *row = a.part + (size_t)blockIdx.x * N;
#pragma unroll
    for (int i = 0; i < NPT; i++) row[tid + WG * i] = acc[i];
}

// sum[p] += part[0][p] + part[1][p] + ... in row order, in double
__global__ __launch_bounds__(WG) void k_scan_reduce(const double *part, int rows, int nfft, double *sum)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nfft) return;
    double s = 0.0;
    for (int r = 0; r < rows; r++) s += part[(size_t)r * nfft + p];
    sum[p] += s;
}

// history for the next push: absolute samples [n1 - T, n1), n1 = n0 + n_in, T = nfft - 1
__global__ __launch_bounds__(WG) void k_scan_history(const void *in, int fmt, long long n0, long long n_in, const float2 *hist_old,
                                                     float2 *hist_new, int T)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= T) return;
    const long long n = n0 + n_in - T + k;
    float2 v;
    if (n >= n0) v = scan_load_new(in, fmt, n - n0);
    else v = hist_old[n - (n0 - T)];                        // n >= n0 - T: the old history holds it (zeros before sample 0)
    hist_new[k] = v;
}

}  // namespace

struct nrsc5hip_scan {
    int device = 0, fmt = 0, nfft = 0, log2n = 0;
    double fs = 0;
    hipStream_t stream = nullptr;
    cplx *d_tw = nullptr;
    float2 *d_hist[2] = {nullptr, nullptr};
    double *d_win = nullptr, *d_part = nullptr, *d_sum = nullptr;
    int cur = 0, part_rows = 0;
    double sum_w2 = 0;
    long long n_total = 0, segments = 0;                    // samples pushed / complete segments since create or reset
};

namespace {
size_t scan_lds_bytes(int nfft) { return sizeof(cplx) * (size_t)(nfft + nfft / 16); }

void free_scan(nrsc5hip_scan *s)
{
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    (void)hipFree(s->d_tw); (void)hipFree(s->d_win); (void)hipFree(s->d_hist[0]); (void)hipFree(s->d_hist[1]);
    (void)hipFree(s->d_part); (void)hipFree(s->d_sum);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int scan_zero_state(nrsc5hip_scan *s)
{
    HIPCHK(hipMemsetAsync(s->d_hist[0], 0, sizeof(float2) * s->nfft, s->stream));
    HIPCHK(hipMemsetAsync(s->d_hist[1], 0, sizeof(float2) * s->nfft, s->stream));
    HIPCHK(hipMemsetAsync(s->d_sum, 0, sizeof(double) * s->nfft, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->cur = 0; s->n_total = 0; s->segments = 0;
    return 0;
}

long long segments_total(const nrsc5hip_scan *s, long long n) { return n < s->nfft ? 0 : (n - s->nfft) / (s->nfft / 2) + 1; }

template <int M> hipError_t scan_set_lds(size_t bytes)
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_scan_psd<M>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <int M> void scan_launch_psd(const ScanArgs &a, int rows, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_psd<M>), dim3((unsigned)rows), dim3(WG), lds, st, a);
}

unsigned bitrev(unsigned v, int bits)
{
    unsigned r = 0;
    for (int i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// ---- detector -----------------------------------------------------------------------------------------------------------------------
// psd[i] is the power of the bin centred at (i - nfft/2) * fs / nfft; the bin covers [i, i + 1) on the axis x(f) = f / bw + nfft/2 + 1/2,
// and the mean power of a frequency interval is the integral of that staircase (a prefix sum plus the two partial bins; x clamped to
// [0, nfft]) over its length.
//   floor      the FLOOR_QUANTILE quantile of the PSD: element (int)(0.2 * (nfft - 1)) of the sorted bins
//   score(c)   for every bin centre c with |c| <= fs/2 - 198.5 kHz: both sidebands [c -+ 198 402, c -+ 129 361] Hz are split into four
//              equal parts; 10 log10(the least of the eight mean powers / floor).  The minimum is what rejects a centre whose windows
//              only partly overlap other stations' sidebands.
//   picks      greedy: highest score first (ties: lower bin), stop below threshold_db, a pick suppresses every centre within
//              +-min_separation_hz of it.  lower_db / upper_db: the whole sidebands' mean power over the floor.
// No edge or flatness test: two analog FM carriers 400 kHz apart can fill both windows of the slot between them, and the decode that
// follows (nrsc5_amd/wideband.py: scan(confirm=True)) is what removes such a nomination.
struct Staircase {
    const double *psd; int nfft; double bw; std::vector<double> pre;
    Staircase(const double *p, int n, double fs) : psd(p), nfft(n), bw(fs / n), pre((size_t)n + 1, 0.0)
    {
        for (int i = 0; i < n; i++) pre[i + 1] = pre[i] + p[i];
    }
    double x_of(double f) const { const double x = f / bw + nfft / 2 + 0.5; return x < 0 ? 0 : x > nfft ? nfft : x; }
    double integral(double x) const
    {
        const int k = (int)floor(x);
        return k >= nfft ? pre[nfft] : pre[k] + (x - k) * psd[k];
    }
    double mean(double f0, double f1) const
    {
        const double x0 = x_of(f0), x1 = x_of(f1);
        return (integral(x1) - integral(x0)) / (x1 - x0);
    }
};

int detect_psd(const double *psd, int nfft, double fs, const nrsc5hip_scan_params *params, nrsc5hip_scan_station *out, int max, int *n_out)
{
    if (!psd || !n_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (nfft < 16 || (nfft & (nfft - 1))) FAIL(NRSC5HIP_EINVAL, "nfft %d is not a power of two >= 16", nfft);
    if (!(fs > 0) || !std::isfinite(fs)) FAIL(NRSC5HIP_EINVAL, "bad sample rate");
    if (max < 0 || (max > 0 && !out)) FAIL(NRSC5HIP_EINVAL, "bad output array (max %d)", max);
    const double threshold = params ? params->threshold_db : 6.0, min_sep = params ? params->min_separation_hz : 100e3;
    if (!std::isfinite(threshold) || !(min_sep >= 0)) FAIL(NRSC5HIP_EINVAL, "bad detector parameters");
    *n_out = 0;
    std::vector<double> sorted(psd, psd + nfft);
    std::sort(sorted.begin(), sorted.end());
    const double floor_p = sorted[(size_t)(FLOOR_QUANTILE * (nfft - 1))];
    if (!(floor_p > 0) || !std::isfinite(floor_p)) return 0;                     // an empty or all-zero capture: nothing to find
    const Staircase st(psd, nfft, fs);
    const double bw = fs / nfft, quarter = (SB_HI_HZ - SB_LO_HZ) / 4;
    struct Cand { double score; int bin; };
    std::vector<Cand> cands;
    for (int i = 0; i < nfft; i++) {
        const double c = (i - nfft / 2) * bw;
        if (!(fabs(c) <= fs / 2 - EDGE_HZ)) continue;
        double least = INFINITY;
        for (int k = 0; k < 4; k++) {
            const double lo = SB_LO_HZ + k * quarter, hi = SB_LO_HZ + (k + 1) * quarter;
            least = fmin(least, fmin(st.mean(c - hi, c - lo), st.mean(c + lo, c + hi)));
        }
        const double score = 10.0 * log10(least / floor_p);
        if (std::isfinite(score) && score >= threshold) cands.push_back({score, i});
    }
    std::sort(cands.begin(), cands.end(), [](const Cand &a, const Cand &b) { return a.score != b.score ? a.score > b.score : a.bin < b.bin; });
    std::vector<double> picked;
    for (const Cand &cd : cands) {
        const double c = (cd.bin - nfft / 2) * bw;
        bool near = false;
        for (double p : picked) if (fabs(p - c) <= min_sep) { near = true; break; }
        if (near) continue;
        if ((int)picked.size() < max) {
            nrsc5hip_scan_station &o = out[picked.size()];
            o.offset_hz = c;
            o.score_db = (float)cd.score;
            o.lower_db = (float)(10.0 * log10(st.mean(c - SB_HI_HZ, c - SB_LO_HZ) / floor_p));
            o.upper_db = (float)(10.0 * log10(st.mean(c + SB_LO_HZ, c + SB_HI_HZ) / floor_p));
            o.floor_db = (float)(10.0 * log10(floor_p));
        }
        picked.push_back(c);
    }
    *n_out = (int)picked.size();
    return 0;
}

// The detector of analog FM carriers (include/nrsc5hip.h): the same floor and Staircase, the score is the mean power of c +- FM_SCORE_HZ over the
// floor, and the reported centre is the centroid of the power above the floor over the bins whose centres lie within FM_CENTROID_HZ of the pick.
// Generous on purpose: a hybrid station's sidebands are nominated as well; measuring the nomination's carrier is what removes them.
constexpr double FM_SCORE_HZ = 50e3, FM_CENTROID_HZ = 100e3, FM_MIN_SEP_HZ = 150e3;

int detect_fm_psd(const double *psd, int nfft, double fs, const nrsc5hip_scan_params *params, nrsc5hip_scan_fm_station *out, int max, int *n_out)
{
    if (!psd || !n_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (nfft < 16 || (nfft & (nfft - 1))) FAIL(NRSC5HIP_EINVAL, "nfft %d is not a power of two >= 16", nfft);
    if (!(fs > 0) || !std::isfinite(fs)) FAIL(NRSC5HIP_EINVAL, "bad sample rate");
    if (max < 0 || (max > 0 && !out)) FAIL(NRSC5HIP_EINVAL, "bad output array (max %d)", max);
    const double threshold = params ? params->threshold_db : 6.0, min_sep = params ? params->min_separation_hz : FM_MIN_SEP_HZ;
    if (!std::isfinite(threshold) || !(min_sep >= 0)) FAIL(NRSC5HIP_EINVAL, "bad detector parameters");
    *n_out = 0;
    std::vector<double> sorted(psd, psd + nfft);
    std::sort(sorted.begin(), sorted.end());
    const double floor_p = sorted[(size_t)(FLOOR_QUANTILE * (nfft - 1))];
    if (!(floor_p > 0) || !std::isfinite(floor_p)) return 0;
    const Staircase st(psd, nfft, fs);
    const double bw = fs / nfft;
    struct Cand { double score; int bin; };
    std::vector<Cand> cands;
    for (int i = 0; i < nfft; i++) {
        const double c = (i - nfft / 2) * bw;
        if (!(fabs(c) <= fs / 2 - EDGE_HZ)) continue;
        const double score = 10.0 * log10(st.mean(c - FM_SCORE_HZ, c + FM_SCORE_HZ) / floor_p);
        if (std::isfinite(score) && score >= threshold) cands.push_back({score, i});
    }
    std::sort(cands.begin(), cands.end(), [](const Cand &a, const Cand &b) { return a.score != b.score ? a.score > b.score : a.bin < b.bin; });
    std::vector<double> picked;
    for (const Cand &cd : cands) {
        const double c = (cd.bin - nfft / 2) * bw;
        bool near = false;
        for (double p : picked) if (fabs(p - c) <= min_sep) { near = true; break; }
        if (near) continue;
        if ((int)picked.size() < max) {
            double sw = 0.0, sfw = 0.0;
            for (int i = 0; i < nfft; i++) {
                const double fi = (i - nfft / 2) * bw;
                if (!(fabs(fi - c) <= FM_CENTROID_HZ)) continue;
                const double w = psd[i] > floor_p ? psd[i] - floor_p : 0.0;
                sw += w; sfw += fi * w;
            }
            nrsc5hip_scan_fm_station &o = out[picked.size()];
            o.offset_hz = sw > 0 ? sfw / sw : c;
            o.bin_hz = c;
            o.score_db = (float)cd.score;
            o.floor_db = (float)(10.0 * log10(floor_p));
        }
        picked.push_back(c);
    }
    *n_out = (int)picked.size();
    return 0;
}
}  // namespace

extern "C" int nrsc5hip_scan_create(const nrsc5hip_scan_config *cfg, nrsc5hip_scan **out)
{
    if (!cfg || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->format < NRSC5HIP_IQ_CU8 || cfg->format > NRSC5HIP_IQ_CF32) FAIL(NRSC5HIP_EINVAL, "bad input format %d", cfg->format);
    if (cfg->rate_num <= 0 || cfg->rate_den <= 0) FAIL(NRSC5HIP_EINVAL, "rate %lld/%lld not positive", cfg->rate_num, cfg->rate_den);
    const __int128 num = cfg->rate_num, den = cfg->rate_den;          // 744 187.5 <= num / den <= 64e6, exactly
    if (num * MIN_RATE_DEN < (__int128)MIN_RATE_NUM * den || num > (__int128)64000000 * den)
        FAIL(NRSC5HIP_EINVAL, "rate %lld/%lld S/s outside 744187.5 .. 64e6", cfg->rate_num, cfg->rate_den);
    const double fs = (double)cfg->rate_num / (double)cfg->rate_den;
    int log2n = 0;
    if (cfg->nfft == 0) {                                             // the smallest power of two >= Fs / 2 kHz, within 512 .. 8192
        for (log2n = MIN_LOG2; log2n < MAX_LOG2 && (double)(1 << log2n) < fs / 2000.0; log2n++) {}
    } else {
        for (log2n = MIN_LOG2; log2n <= MAX_LOG2 && (1 << log2n) != cfg->nfft; log2n++) {}
        if (log2n > MAX_LOG2) FAIL(NRSC5HIP_EINVAL, "nfft %d is not a power of two in 512..8192", cfg->nfft);
    }
    const int nfft = 1 << log2n;

    nrsc5hip_scan *s = new (std::nothrow) nrsc5hip_scan;
    if (!s) FAIL(NRSC5HIP_ENOMEM, "out of host memory");
    s->device = cfg->device; s->fmt = cfg->format; s->nfft = nfft; s->log2n = log2n; s->fs = fs;
    std::vector<cplx> tw(nfft);
    std::vector<double> win(nfft);
    for (int k = 0; k < nfft; k++) {
        const double ph = 2.0 * M_PI * k / nfft;
        tw[k].x = cos(ph); tw[k].y = -sin(ph);
        win[k] = 0.5 - 0.5 * cos(ph);
        s->sum_w2 += win[k] * win[k];
    }

    nrsc5::DeviceGuard guard(s->device);
#define CREATE_CHK(expr) HIPCHK_OR(expr, free_scan(s))
    CREATE_CHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    CREATE_CHK(hipMalloc(&s->d_tw, sizeof(cplx) * nfft));
    CREATE_CHK(hipMalloc(&s->d_win, sizeof(double) * nfft));
    CREATE_CHK(hipMalloc(&s->d_hist[0], sizeof(float2) * nfft));
    CREATE_CHK(hipMalloc(&s->d_hist[1], sizeof(float2) * nfft));
    CREATE_CHK(hipMalloc(&s->d_sum, sizeof(double) * nfft));
    CREATE_CHK(hipMemcpy(s->d_tw, tw.data(), sizeof(cplx) * nfft, hipMemcpyHostToDevice));
    CREATE_CHK(hipMemcpy(s->d_win, win.data(), sizeof(double) * nfft, hipMemcpyHostToDevice));
    const size_t lds = scan_lds_bytes(nfft);
    switch (log2n) {
    case 9: CREATE_CHK(scan_set_lds<9>(lds)); break;
    case 10: CREATE_CHK(scan_set_lds<10>(lds)); break;
    case 11: CREATE_CHK(scan_set_lds<11>(lds)); break;
    case 12: CREATE_CHK(scan_set_lds<12>(lds)); break;
    default: CREATE_CHK(scan_set_lds<13>(lds)); break;
    }
#undef CREATE_CHK
    int rc = scan_zero_state(s);
    if (rc) { free_scan(s); return rc; }
    *out = s;
    return 0;
}

extern "C" void nrsc5hip_scan_destroy(nrsc5hip_scan *s)
{
    if (!s) return;
    nrsc5::DeviceGuard guard(s->device);
    free_scan(s);
}

extern "C" int nrsc5hip_scan_reset(nrsc5hip_scan *s)
{
    if (!s) FAIL(NRSC5HIP_EINVAL, "null scanner");
    nrsc5::DeviceGuard guard(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    return scan_zero_state(s);
}

extern "C" int nrsc5hip_scan_push(nrsc5hip_scan *s, const void *dev_in, long long n_in)
{
    if (!s) FAIL(NRSC5HIP_EINVAL, "null scanner");
    if (n_in < 0 || (n_in > 0 && !dev_in)) FAIL(NRSC5HIP_EINVAL, "bad input (n_in %lld)", n_in);
    if (n_in == 0) return 0;
    const long long nseg = segments_total(s, s->n_total + n_in) - s->segments;
    if (nseg > 0x7fffffffLL) FAIL(NRSC5HIP_EINVAL, "push too large: %lld segments", nseg);
    nrsc5::DeviceGuard guard(s->device);
    if (nseg > 0) {
        int run = (int)((nseg + ROWS_TARGET - 1) / ROWS_TARGET);
        if (run > RUN_MAX) run = RUN_MAX;
        const int rows = (int)((nseg + run - 1) / run);
        if (rows > s->part_rows) {
            HIPCHK(hipStreamSynchronize(s->stream));
            HIPCHK(hipFree(s->d_part)); s->d_part = nullptr; s->part_rows = 0;
            HIPCHK(hipMalloc(&s->d_part, sizeof(double) * (size_t)rows * s->nfft));
            s->part_rows = rows;
        }
        ScanArgs a;
        a.in = dev_in; a.fmt = s->fmt; a.n0 = s->n_total; a.n_in = n_in; a.hist = s->d_hist[s->cur]; a.tw = s->d_tw; a.win = s->d_win;
        a.seg0 = s->segments; a.nseg = (int)nseg; a.run = run; a.part = s->d_part;
        const size_t lds = scan_lds_bytes(s->nfft);
        switch (s->log2n) {
        case 9: scan_launch_psd<9>(a, rows, lds, s->stream); break;
        case 10: scan_launch_psd<10>(a, rows, lds, s->stream); break;
        case 11: scan_launch_psd<11>(a, rows, lds, s->stream); break;
        case 12: scan_launch_psd<12>(a, rows, lds, s->stream); break;
        default: scan_launch_psd<13>(a, rows, lds, s->stream); break;
        }
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_scan_reduce, dim3((s->nfft + WG - 1) / WG), dim3(WG), 0, s->stream, (const double *)s->d_part, rows, s->nfft, s->d_sum);
        HIPCHK(hipGetLastError());
    }
    const int T = s->nfft - 1;
    hipLaunchKernelGGL(k_scan_history, dim3((T + WG - 1) / WG), dim3(WG), 0, s->stream, dev_in, s->fmt, s->n_total, n_in,
                       (const float2 *)s->d_hist[s->cur], s->d_hist[s->cur ^ 1], T);
    HIPCHK(hipGetLastError());
    s->cur ^= 1;
    s->n_total += n_in;
    s->segments += nseg;
    HIPCHK(hipStreamSynchronize(s->stream));               // dev_in no longer read when the call returns
    return 0;
}

extern "C" int nrsc5hip_scan_info(nrsc5hip_scan *s, int *nfft, long long *segments, double *bin_hz)
{
    if (!s) FAIL(NRSC5HIP_EINVAL, "null scanner");
    if (nfft) *nfft = s->nfft;
    if (segments) *segments = s->segments;
    if (bin_hz) *bin_hz = s->fs / s->nfft;
    return 0;
}

extern "C" int nrsc5hip_scan_spectrum(nrsc5hip_scan *s, double *psd)
{
    if (!s || !psd) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (s->segments == 0) FAIL(NRSC5HIP_EINVAL, "no complete segment yet (%lld of %d samples)", s->n_total, s->nfft);
    nrsc5::DeviceGuard guard(s->device);
    std::vector<double> sum(s->nfft);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(sum.data(), s->d_sum, sizeof(double) * s->nfft, hipMemcpyDeviceToHost));
    const double scale = 1.0 / ((double)s->segments * s->sum_w2);
    for (int p = 0; p < s->nfft; p++) {
        const int k = (int)bitrev((unsigned)p, s->log2n);
        psd[(k + s->nfft / 2) & (s->nfft - 1)] = sum[p] * scale;
    }
    return 0;
}

extern "C" int nrsc5hip_scan_detect_psd(const double *psd, int nfft, double fs, const nrsc5hip_scan_params *params,
                                        nrsc5hip_scan_station *stations_out, int max, int *n)
{
    return detect_psd(psd, nfft, fs, params, stations_out, max, n);
}

extern "C" int nrsc5hip_scan_detect_fm_psd(const double *psd, int nfft, double fs, const nrsc5hip_scan_params *params,
                                           nrsc5hip_scan_fm_station *stations_out, int max, int *n)
{
    return detect_fm_psd(psd, nfft, fs, params, stations_out, max, n);
}

extern "C" int nrsc5hip_scan_detect_fm(nrsc5hip_scan *s, const nrsc5hip_scan_params *params, nrsc5hip_scan_fm_station *stations_out, int max, int *n)
{
    if (!s || !n) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (max < 0 || (max > 0 && !stations_out)) FAIL(NRSC5HIP_EINVAL, "bad output array (max %d)", max);
    std::vector<double> psd(s->nfft);
    int rc = nrsc5hip_scan_spectrum(s, psd.data());
    if (rc) return rc;
    return detect_fm_psd(psd.data(), s->nfft, s->fs, params, stations_out, max, n);
}

extern "C" int nrsc5hip_scan_detect(nrsc5hip_scan *s, const nrsc5hip_scan_params *params, nrsc5hip_scan_station *stations_out, int max, int *n)
{
    if (!s || !n) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (max < 0 || (max > 0 && !stations_out)) FAIL(NRSC5HIP_EINVAL, "bad output array (max %d)", max);
    std::vector<double> psd(s->nfft);
    int rc = nrsc5hip_scan_spectrum(s, psd.data());
    if (rc) return rc;
    return detect_psd(psd.data(), s->nfft, s->fs, params, stations_out, max, n);
}
