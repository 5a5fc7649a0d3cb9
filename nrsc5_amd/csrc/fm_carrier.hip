// Carrier quality of the analog host, host side (include/nrsc5hip.h, "carrier quality"): the buffers an analog FM object gains
// with nrsc5hip_fm_carrier_enable, the launches fm_launch chains behind its audio, the figures formed from the sums, and the stage hook.  The
// kernels are in k_fm_carrier.hip (and k_fm_front, which writes r).
//   per push, host -> device: nothing (the launches carry their arguments)
//   per nrsc5hip_fm_carrier, device -> host: 48 bytes per channel (the two triples)
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "nrsc5hip.h"
#include "host_util.h"
#include "arena_consumer.h"
#include "fm_audio.h"

using namespace nrsc5;
using namespace nrsc5::fm;

struct nrsc5::CarrierHost {
    float *d_r[2] = {nullptr, nullptr}; long long r_cap = 0;      // r[m], m in [540 blocks, m_total), of channel c at d_r[cur][c * r_cap + m - 540 blocks]
    double *d_t[2] = {nullptr, nullptr}; long long t_cap = 0, t_base = 0;   // block triples [t_base, blocks) at d_t[cur][3 * (c * t_cap + j - t_base)]
    int cur = 0;
    DevFixed<double> d_report;                                    // [nchan][6]
    double wsum = 0;                                              // sum of the window as the device reads it: the windowed report's count
    ~CarrierHost() { for (int i = 0; i < 2; i++) { (void)hipFree(d_r[i]); (void)hipFree(d_t[i]); } }
};

namespace {

void figures(nrsc5hip_fm_carrier_report &o)
{
    o.level_db = o.cnr_db = o.offset_hz = 0.0;
    if (!(o.count > 0)) return;
    const double P = o.sum2 / (540.0 * o.count), K = o.sum4 / (540.0 * o.count);   // means per sample: count is in blocks
    const double q = 2.0 * P * P - K, S = q > 0 ? sqrt(q) : 0.0, N = P - S;
    const double lo = NRSC5HIP_FM_CARRIER_DB_MIN, hi = NRSC5HIP_FM_CARRIER_DB_MAX;
    double level = lo, cnr = lo;
    if (S > 0 && P > 0) {
        level = 10.0 * log10(S / (32768.0 * 32768.0));
        cnr = N > 0 ? 10.0 * log10(S / N) : hi;
    }
    o.level_db = level < lo ? lo : level > hi ? hi : level;
    o.cnr_db = cnr < lo ? lo : cnr > hi ? hi : cnr;
    o.offset_hz = 75000.0 * o.sum1 / (540.0 * o.count);
}

}  // namespace

void nrsc5::carrier_free(CarrierHost *c) { delete c; }

int nrsc5::carrier_reset(nrsc5hip_fm *f)
{
    CarrierHost *C = f->carrier;
    HIPCHK(hipMemsetAsync(C->d_report.p, 0, sizeof(double) * 6 * f->nchan, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    C->cur = 0; C->t_base = 0;
    return 0;
}

int nrsc5::carrier_reserve(nrsc5hip_fm *f, hipStream_t s, long long m1, long long b1)
{
    CarrierHost *C = f->carrier;
    const long long r_base = (long long)BLOCK * f->blocks, need_r = m1 - r_base, need_t = b1 - C->t_base;
    if (need_r > C->r_cap) {
        HIPCHK(hipStreamSynchronize(s));
        const long long cap = need_r + need_r / 4 + 4096;
        float *nr[2] = {nullptr, nullptr};
        HIPCHK(hipMalloc(&nr[0], sizeof(float) * (size_t)cap * f->nchan));
        if (hipMalloc(&nr[1], sizeof(float) * (size_t)cap * f->nchan) != hipSuccess) { (void)hipFree(nr[0]); FAIL(NRSC5HIP_ENOMEM, "out of device memory (r, %lld per channel)", cap); }
        const long long have = f->m_total - r_base;
        if (have > 0)
            HIPCHK(hipMemcpy2DAsync(nr[C->cur], sizeof(float) * cap, C->d_r[C->cur], sizeof(float) * C->r_cap, sizeof(float) * have, f->nchan, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        (void)hipFree(C->d_r[0]); (void)hipFree(C->d_r[1]);
        C->d_r[0] = nr[0]; C->d_r[1] = nr[1]; C->r_cap = cap;
    }
    if (need_t > C->t_cap) {
        HIPCHK(hipStreamSynchronize(s));
        const long long cap = need_t + need_t / 4 + 64;
        double *nt[2] = {nullptr, nullptr};
        HIPCHK(hipMalloc(&nt[0], sizeof(double) * 3 * (size_t)cap * f->nchan));
        if (hipMalloc(&nt[1], sizeof(double) * 3 * (size_t)cap * f->nchan) != hipSuccess) { (void)hipFree(nt[0]); FAIL(NRSC5HIP_ENOMEM, "out of device memory (carrier sums)"); }
        const long long have = f->blocks - C->t_base;
        if (have > 0)
            HIPCHK(hipMemcpy2DAsync(nt[C->cur], sizeof(double) * 3 * cap, C->d_t[C->cur], sizeof(double) * 3 * C->t_cap, sizeof(double) * 3 * have, f->nchan, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        (void)hipFree(C->d_t[0]); (void)hipFree(C->d_t[1]);
        C->d_t[0] = nt[0]; C->d_t[1] = nt[1]; C->t_cap = cap;
    }
    return 0;
}

nrsc5::FrontTarget nrsc5::carrier_front(const nrsc5hip_fm *f)
{
    const CarrierHost *C = f->carrier;
    return FrontTarget{C->d_r[C->cur], C->r_cap, (long long)BLOCK * f->blocks};
}

int nrsc5::carrier_launch_sums(nrsc5hip_fm *f, hipStream_t s, const float *d, long long b1)
{
    CarrierHost *C = f->carrier;
    CarrierArgs a;
    a.r = C->d_r[C->cur]; a.r_stride = C->r_cap; a.r_base = (long long)BLOCK * f->blocks;
    a.d = d; a.d_stride = f->d_cap; a.d_base = f->d_base;
    a.t = C->d_t[C->cur]; a.t_stride = C->t_cap; a.t_base = C->t_base; a.j0 = f->blocks;
    launch_carrier(s, (int)(b1 - f->blocks), f->nchan, a);
    HIPCHK(hipGetLastError());
    return 0;
}

nrsc5::Triples nrsc5::carrier_triples(const nrsc5hip_fm *f)
{
    const CarrierHost *C = f->carrier;
    return Triples{C->d_t[C->cur], C->t_cap, C->t_base};
}

int nrsc5::carrier_launch_report(nrsc5hip_fm *f, hipStream_t s, long long m1, long long b1, long long a1)
{
    CarrierHost *C = f->carrier;
    const long long r_base = (long long)BLOCK * f->blocks;
    ReportArgs q;
    q.t = C->d_t[C->cur]; q.t_new = C->d_t[C->cur ^ 1]; q.t_stride = C->t_cap; q.t_base = C->t_base;
    q.t_base_new = b1 > TRIPLES_KEPT ? b1 - TRIPLES_KEPT : 0;
    q.j0 = f->blocks; q.j1 = b1; q.ja = a1 - 1; q.win = f->d_win; q.report = C->d_report.p;
    q.r_old = C->d_r[C->cur]; q.r_new = C->d_r[C->cur ^ 1]; q.r_stride = C->r_cap; q.r_shift = (long long)BLOCK * b1 - r_base; q.r_count = m1 - (long long)BLOCK * b1;
    launch_carrier_report(s, f->nchan, q);
    HIPCHK(hipGetLastError());
    C->cur ^= 1; C->t_base = q.t_base_new;
    return 0;
}

extern "C" int nrsc5hip_fm_carrier_enable(nrsc5hip_fm *f)
{
    if (!f) FAIL(NRSC5HIP_EINVAL, "null demodulator");
    if (f->carrier) FAIL(NRSC5HIP_EINVAL, "the carrier measurement is enabled already");
    if (f->processed) FAIL(NRSC5HIP_EINVAL, "the carrier measurement can be enabled only before the first push");
    return nrsc5::carrier_enable(f);
}

int nrsc5::carrier_enable(nrsc5hip_fm *f)
{
    static_assert(TRIPLES_KEPT >= 2 * W + 1, "the steered audio kernel reads the window of the audio block in front of the push");
    nrsc5::DeviceGuard guard(f->device);
    CarrierHost *C = new (std::nothrow) CarrierHost;
    if (!C) FAIL(NRSC5HIP_ENOMEM, "out of host memory");
    for (int w = -W; w <= W; w++) C->wsum += (double)(float)(0.5 * (1 + cos(M_PI * w / (W + 1))));
    const size_t K = (size_t)f->nchan;
    C->r_cap = BLOCK + 65536;
    C->t_cap = TRIPLES_KEPT + 256;
#define ENABLE_CHK(expr) HIPCHK_OR(expr, delete C)
    for (int i = 0; i < 2; i++) {
        ENABLE_CHK(hipMalloc(&C->d_r[i], sizeof(float) * (size_t)C->r_cap * K));
        ENABLE_CHK(hipMalloc(&C->d_t[i], sizeof(double) * 3 * (size_t)C->t_cap * K));
    }
    ENABLE_CHK(hipMalloc(&C->d_report.p, sizeof(double) * 6 * K));
#undef ENABLE_CHK
    f->carrier = C;
    const int rc = carrier_reset(f);
    if (rc) { f->carrier = nullptr; delete C; }
    return rc;
}

extern "C" int nrsc5hip_fm_carrier(nrsc5hip_fm *f, nrsc5hip_fm_carrier_info *out)
{
    if (!f || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (!f->carrier) FAIL(NRSC5HIP_EINVAL, "the carrier measurement is not enabled on this object");
    nrsc5::DeviceGuard guard(f->device);
    CarrierHost *C = f->carrier;
    std::vector<double> v(6 * (size_t)f->nchan);
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpy(v.data(), C->d_report.p, sizeof(double) * v.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < f->nchan; k++) {
        nrsc5hip_fm_carrier_info &o = out[k];
        memset(&o, 0, sizeof(o));
        o.blocks = f->blocks; o.audio_blocks = f->audio_blocks;
        if (f->audio_blocks > 0) { o.windowed.sum2 = v[6 * k]; o.windowed.sum4 = v[6 * k + 1]; o.windowed.sum1 = v[6 * k + 2]; o.windowed.count = C->wsum; }
        if (f->blocks > 0) { o.running.sum2 = v[6 * k + 3]; o.running.sum4 = v[6 * k + 4]; o.running.sum1 = v[6 * k + 5]; o.running.count = (double)f->blocks; }
        figures(o.windowed); figures(o.running);
    }
    return 0;
}

extern "C" int nrsc5hip_stage_fm_carrier(nrsc5hip_fm *f, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *r_out, double *sums_out)
{
    if (!f || !r_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (n_in <= 0 || !dev_in) FAIL(NRSC5HIP_EINVAL, "bad input (n_in %lld)", n_in);
    if (((uintptr_t)dev_in & 3) || (in_stride_elems & 1)) FAIL(NRSC5HIP_EINVAL, "input not aligned to 4 bytes (in_stride_elems %lld)", in_stride_elems);
    if (f->nchan > 1 && in_stride_elems < 2 * n_in) FAIL(NRSC5HIP_EINVAL, "in_stride_elems %lld < 2 * n_in %lld", in_stride_elems, n_in);
    const long long m1 = (n_in + 1) >> 1, b1 = m1 / BLOCK;
    if ((m1 + FT - 1) / FT > 0x7fffffffLL) FAIL(NRSC5HIP_EINVAL, "input too large (%lld samples)", n_in);
    const size_t K = (size_t)f->nchan;
    nrsc5::DeviceGuard guard(f->device);
    nrsc5::DevTmp d, r, t, hist;
    HIPCHK(hipMalloc(&d.p, sizeof(float) * (size_t)m1 * K));
    HIPCHK(hipMalloc(&r.p, sizeof(float) * (size_t)m1 * K));
    HIPCHK(hipMalloc(&t.p, sizeof(double) * 3 * (size_t)(b1 + 1) * K));
    HIPCHK(hipMalloc(&hist.p, sizeof(int) * HIST * K));
    HIPCHK(hipMemsetAsync(hist.p, 0, sizeof(int) * HIST * K, f->stream));
    FrontArgs a;
    a.in = dev_in; a.in_stride = in_stride_elems; a.n0 = 0; a.n_in = n_in; a.hist = (const int *)hist.p; a.ha = f->d_ha;
    a.d = (float *)d.p; a.d_stride = m1; a.d_base = 0; a.m0 = 0; a.m_count = m1;
    a.r = (float *)r.p; a.r_stride = m1; a.r_base = 0;
    launch_front(f->stream, (int)((m1 + FT - 1) / FT), f->nchan, a);
    HIPCHK(hipGetLastError());
    if (b1 > 0) {
        CarrierArgs q;
        q.r = (const float *)r.p; q.r_stride = m1; q.r_base = 0; q.d = (const float *)d.p; q.d_stride = m1; q.d_base = 0;
        q.t = (double *)t.p; q.t_stride = b1; q.t_base = 0; q.j0 = 0;
        launch_carrier(f->stream, (int)b1, f->nchan, q);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpy(r_out, r.p, sizeof(float) * (size_t)m1 * K, hipMemcpyDeviceToHost));
    if (sums_out && b1 > 0) HIPCHK(hipMemcpy(sums_out, t.p, sizeof(double) * 3 * (size_t)b1 * K, hipMemcpyDeviceToHost));
    return 0;
}
