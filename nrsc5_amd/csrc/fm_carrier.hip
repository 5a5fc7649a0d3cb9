// Carrier quality of the analog host, host side (include/nrsc5hip.h, "carrier quality"): the buffers an analog FM object gains
// with nrsc5hip_fm_carrier_enable, the launches fm_launch chains behind its audio, the figures formed from the sums, and the stage hook.  The
// kernels are in k_fm_carrier.hip (and k_fm_front, which writes r); the buffers that grow, the hook's opening and the dB clamp are fm_host.h's.
//   per push, host -> device: nothing (the launches carry their arguments)
//   per nrsc5hip_fm_carrier, device -> host: 48 bytes per channel (the two triples)
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "nrsc5hip.h"
#include "host_util.h"
#include "fm_host.h"

using namespace nrsc5;
using namespace nrsc5::fm;

struct nrsc5::CarrierHost {
    PingPong<float> r;                                            // r[m], m in [540 blocks, m_total), of channel c at r.p[cur][c * r.cap + m - 540 blocks]
    PingPong<double> t; long long t_base = 0;                     // block triples [t_base, blocks) at t.p[cur][3 * (c * t.cap + j - t_base)]
    int cur = 0;                                                  // of r and t
    DevFixed<double> d_report;                                    // [nchan][6]
    double wsum = 0;                                              // sum of the window as the device reads it: the windowed report's count
};

namespace {

void figures(nrsc5hip_fm_carrier_report &o)
{
    o.level_db = o.cnr_db = o.offset_hz = 0.0;
    if (!(o.count > 0)) return;
    const double P = o.sum2 / (540.0 * o.count), K = o.sum4 / (540.0 * o.count);   // means per sample: count is in blocks
    const double q = 2.0 * P * P - K, S = q > 0 ? sqrt(q) : 0.0, N = P - S;
    o.level_db = o.cnr_db = NRSC5HIP_FM_CARRIER_DB_MIN;
    if (S > 0 && P > 0) {
        o.level_db = clamp_db(10.0 * log10(S / (32768.0 * 32768.0)));
        o.cnr_db = N > 0 ? clamp_db(10.0 * log10(S / N)) : NRSC5HIP_FM_CARRIER_DB_MAX;
    }
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
    const long long r_base = (long long)BLOCK * f->blocks;
    const int rc = C->r.reserve(s, m1 - r_base, f->m_total - r_base, f->nchan, 1, 4096, C->cur, "r");
    return rc ? rc : C->t.reserve(s, b1 - C->t_base, f->blocks - C->t_base, f->nchan, 3, 64, C->cur, "carrier sums");
}

nrsc5::FrontTarget nrsc5::carrier_front(const nrsc5hip_fm *f)
{
    const CarrierHost *C = f->carrier;
    return FrontTarget{C->r.p[C->cur], C->r.cap, (long long)BLOCK * f->blocks};
}

int nrsc5::carrier_launch_sums(nrsc5hip_fm *f, hipStream_t s, const float *d, long long b1)
{
    CarrierHost *C = f->carrier;
    CarrierArgs a;
    a.r = C->r.p[C->cur]; a.r_stride = C->r.cap; a.r_base = (long long)BLOCK * f->blocks;
    a.d = d; a.d_stride = f->d.cap; a.d_base = f->d_base;
    a.t = C->t.p[C->cur]; a.t_stride = C->t.cap; a.t_base = C->t_base; a.j0 = f->blocks;
    launch_carrier(s, (int)(b1 - f->blocks), f->nchan, a);
    HIPCHK(hipGetLastError());
    return 0;
}

nrsc5::Triples nrsc5::carrier_triples(const nrsc5hip_fm *f)
{
    const CarrierHost *C = f->carrier;
    return Triples{C->t.p[C->cur], C->t.cap, C->t_base};
}

int nrsc5::carrier_launch_report(nrsc5hip_fm *f, hipStream_t s, long long m1, long long b1, long long a1)
{
    CarrierHost *C = f->carrier;
    const long long r_base = (long long)BLOCK * f->blocks;
    ReportArgs q;
    q.t = C->t.p[C->cur]; q.t_new = C->t.p[C->cur ^ 1]; q.t_stride = C->t.cap; q.t_base = C->t_base;
    q.t_base_new = b1 > TRIPLES_KEPT ? b1 - TRIPLES_KEPT : 0;
    q.j0 = f->blocks; q.j1 = b1; q.ja = a1 - 1; q.win = f->d_win; q.report = C->d_report.p;
    q.r_old = C->r.p[C->cur]; q.r_new = C->r.p[C->cur ^ 1]; q.r_stride = C->r.cap; q.r_shift = (long long)BLOCK * b1 - r_base; q.r_count = m1 - (long long)BLOCK * b1;
    launch_carrier_report(s, f->nchan, q);
    HIPCHK(hipGetLastError());
    C->cur ^= 1; C->t_base = q.t_base_new;
    return 0;
}

extern "C" int nrsc5hip_fm_carrier_enable(nrsc5hip_fm *f)
{
    FM_ENABLE_CHECK(f, f->carrier, "the carrier measurement");
    return nrsc5::carrier_enable(f);
}

int nrsc5::carrier_enable(nrsc5hip_fm *f)
{
    static_assert(TRIPLES_KEPT >= 2 * W + 1, "the steered audio kernel reads the window of the audio block in front of the push");
    nrsc5::DeviceGuard guard(f->device);
    CarrierHost *C = new (std::nothrow) CarrierHost;
    if (!C) FAIL(NRSC5HIP_ENOMEM, "out of host memory");
    for (float v : hann_window()) C->wsum += (double)v;
#define ENABLE_CHK(expr) HIPCHK_OR(expr, delete C)
    ENABLE_CHK(C->r.alloc(BLOCK + 65536, f->nchan));
    ENABLE_CHK(C->t.alloc(TRIPLES_KEPT + 256, f->nchan, 3));
    ENABLE_CHK(hipMalloc(&C->d_report.p, sizeof(double) * 6 * (size_t)f->nchan));
#undef ENABLE_CHK
    f->carrier = C;
    const int rc = carrier_reset(f);
    if (rc) { f->carrier = nullptr; delete C; }
    return rc;
}

extern "C" int nrsc5hip_fm_carrier(nrsc5hip_fm *f, nrsc5hip_fm_carrier_info *out)
{
    if (!f || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    FM_FEATURE_ENTER(f, carrier, "the carrier measurement");
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
    nrsc5::DeviceGuard guard(f->device);
    StageFront sf;
    const int rc = sf.open(f, dev_in, in_stride_elems, n_in, true);
    if (rc) return rc;
    const long long m1 = sf.m1, b1 = sf.b1;
    const size_t K = (size_t)f->nchan;
    nrsc5::DevTmp t;
    HIPCHK(hipMalloc(&t.p, sizeof(double) * 3 * (size_t)(b1 + 1) * K));
    if (b1 > 0) {
        CarrierArgs q;
        q.r = sf.rf(); q.r_stride = m1; q.r_base = 0; q.d = sf.df(); q.d_stride = m1; q.d_base = 0;
        q.t = (double *)t.p; q.t_stride = b1; q.t_base = 0; q.j0 = 0;
        launch_carrier(f->stream, (int)b1, f->nchan, q);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpy(r_out, sf.r.p, sizeof(float) * (size_t)m1 * K, hipMemcpyDeviceToHost));
    if (sums_out && b1 > 0) HIPCHK(hipMemcpy(sums_out, t.p, sizeof(double) * 3 * (size_t)b1 * K, hipMemcpyDeviceToHost));
    return 0;
}
