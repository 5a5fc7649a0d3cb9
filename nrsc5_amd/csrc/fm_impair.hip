// Reception impairments of the analog host, host side (include/nrsc5hip.h, "reception impairments"): the band-pass design in
// double, the buffers an analog FM object gains with nrsc5hip_fm_impair_enable, the two launches fm_launch chains behind the carrier sums, the
// figures and the verdict formed from the sums, and the stage hook.  The kernels are in k_fm_impair.hip; the records' buffer that grows, the hook's
// opening and the dB clamp are fm_host.h's.
//   per push, host -> device: nothing (the launches carry their arguments)
//   per nrsc5hip_fm_impair, device -> host: 176 bytes per channel (the two sets of eleven sums)
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

struct nrsc5::ImpairHost {
    PingPong<double> t; long long t_base = 0;                     // block records [t_base, blocks) at t.p[cur][NS * (c * t.cap + j - t_base)]
    int cur = 0;
    double *d_report = nullptr;                                   // [nchan][2 NS]
    float *d_tail = nullptr;                                      // [nchan][R_TAIL]: r[540 blocks - R_TAIL, 540 blocks)
    float *d_hu = nullptr;                                        // [UT]
    nrsc5hip_fm_impair_config cfg = {0.5, 0.05, 0.5};
    double wsum = 0;                                              // sum of the window as the device reads it: the windowed report's count
    ~ImpairHost() { (void)hipFree(d_report); (void)hipFree(d_tail); (void)hipFree(d_hu); }
};

namespace {

constexpr double FS1 = 744187.5 / 2, EDGE_LO = 100e3, EDGE_HI = 170e3, BETA = 8.0;

// hU as stored: designed once; the getter, the enabled object's device table and the stage hook all read this one table
const std::vector<float> &hu_table();

// Kaiser-windowed difference of two sincs, symmetric about tap 31 (the window's end taps are 1 / I0(beta), not fm_audio.hip's design)
std::vector<float> design_hu()
{
    const double f1 = EDGE_LO / FS1, f2 = EDGE_HI / FS1, i0b = bessel_i0(BETA);
    std::vector<float> h(UT);
    for (int i = 0; i < UT; i++) {
        const double tau = i - 0.5 * (UT - 1), u = 2.0 * tau / (UT - 1);
        const double w = fabs(u) < 1.0 ? bessel_i0(BETA * sqrt(1.0 - u * u)) / i0b : 1.0 / i0b;
        h[i] = (float)((2.0 * f2 * sinc(2.0 * f2 * tau) - 2.0 * f1 * sinc(2.0 * f1 * tau)) * w);
    }
    return h;
}

const std::vector<float> &hu_table()
{
    static const std::vector<float> h = design_hu();
    return h;
}

// the figures and the verdict of one set of sums, line by line as include/nrsc5hip.h states them
void figures(nrsc5hip_fm_impair_report &o, const nrsc5hip_fm_impair_config &cfg)
{
    o.explained = o.depth = o.slope = o.curvature = o.usn_db = o.ripple_db = o.rho = 0.0;
    o.verdict = o.side = 0;
    if (!(o.count > 0)) return;
    const double n = 540.0 * o.count;
    const double mx = o.sx / n, m2 = o.sxx / n, m3 = o.sxxx / n, m4 = o.sxxxx / n, my = o.sy / n, mxy = o.sxy / n, mxxy = o.sxxy / n, myy = o.syy / n;
    const double q = mx * mx;
    const double u2 = m2 - q;
    const double u3 = (m3 - (3.0 * mx) * m2) + (2.0 * mx) * q;
    const double u4 = ((m4 - (4.0 * mx) * m3) + (6.0 * q) * m2) - (3.0 * q) * q;
    const double cu = mxy - mx * my;
    const double cv = ((mxxy - (2.0 * mx) * mxy) + q * my) - u2 * my;
    const double k = u4 - u2 * u2;
    const double det = u2 * k - u3 * u3;
    const double tot = myy - my * my;
    if (my > 0 && tot > 0 && u2 >= NRSC5HIP_FM_IMPAIR_MOD_MIN && det >= NRSC5HIP_FM_IMPAIR_MOD_MIN * ((u2 * u2) * u2)) {
        const double b1 = (cu * k - cv * u3) / det, b2 = (cv * u2 - cu * u3) / det;
        const double res = tot - (b1 * cu + b2 * cv);
        const double ex = 1.0 - res / tot, fit = tot - res;
        const double c1 = b1 - (2.0 * b2) * mx, c0 = (my - b1 * mx) + b2 * (q - u2);
        const double explained = ex < 0.0 ? 0.0 : ex > 1.0 ? 1.0 : ex;
        const double depth = sqrt(fit > 0.0 ? fit : 0.0) / my;
        const double slope = c0 > 0 ? c1 / c0 : 0.0, curvature = c0 > 0 ? b2 / c0 : 0.0;
        if (std::isfinite(ex) && std::isfinite(depth) && std::isfinite(slope) && std::isfinite(curvature)) {
            o.explained = explained; o.depth = depth; o.slope = slope; o.curvature = curvature;
        }
    }
    const double lo = NRSC5HIP_FM_CARRIER_DB_MIN;
    o.usn_db = o.cdd > 0 ? clamp_db(10.0 * log10(o.cdd / n)) : lo;
    o.ripple_db = o.cee > 0 && my > 0 ? clamp_db(10.0 * log10((o.cee / n) / (my * my))) : lo;
    if (o.cee > 0 && o.cdd > 0) {
        const double rho = o.ced / sqrt(o.cee * o.cdd);
        o.rho = !std::isfinite(rho) ? 0.0 : rho < -1.0 ? -1.0 : rho > 1.0 ? 1.0 : rho;
    }
    if (o.explained >= cfg.explained_min && o.depth >= cfg.depth_min) o.verdict |= NRSC5HIP_FM_IMPAIR_MULTIPATH;
    if (fabs(o.rho) >= cfg.rho_min && o.rho != 0.0) { o.verdict |= NRSC5HIP_FM_IMPAIR_ADJACENT; o.side = o.rho > 0 ? 1 : -1; }
}

void fill(nrsc5hip_fm_impair_report &o, const double *v, double count)
{
    o.sx = v[0]; o.sxx = v[1]; o.sxxx = v[2]; o.sxxxx = v[3]; o.sy = v[4]; o.sxy = v[5]; o.sxxy = v[6]; o.syy = v[7];
    o.cee = v[8]; o.cdd = v[9]; o.ced = v[10]; o.count = count;
}

}  // namespace

void nrsc5::impair_free(ImpairHost *p) { delete p; }

int nrsc5::impair_reset(nrsc5hip_fm *f)
{
    ImpairHost *P = f->impair;
    HIPCHK(hipMemsetAsync(P->d_report, 0, sizeof(double) * 2 * NS * f->nchan, f->stream));
    HIPCHK(hipMemsetAsync(P->d_tail, 0, sizeof(float) * R_TAIL * f->nchan, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    P->cur = 0; P->t_base = 0;
    return 0;
}

int nrsc5::impair_reserve(nrsc5hip_fm *f, hipStream_t s, long long b1)
{
    ImpairHost *P = f->impair;
    return P->t.reserve(s, b1 - P->t_base, f->blocks - P->t_base, f->nchan, NS, 64, P->cur, "impairment sums");
}

int nrsc5::impair_launch(nrsc5hip_fm *f, hipStream_t s, const float *d, long long b1, long long a1)
{
    ImpairHost *P = f->impair;
    const FrontTarget r = carrier_front(f);                   // this push's r: from the first sample of the first new block on
    const long long first = (long long)BLOCK * f->blocks - (UT - 1);
    if (f->d_base > (first > 0 ? first : 0)) FAIL(NRSC5HIP_EHIP, "internal: d is kept from %lld, the impairment sums read from %lld", f->d_base, first);
    ImpairArgs a;
    a.r = r.r; a.r_stride = r.r_stride; a.r_base = r.r_base; a.r_tail = P->d_tail;
    a.d = d; a.d_stride = f->d.cap; a.d_base = f->d_base; a.hu = P->d_hu;
    a.t = P->t.p[P->cur]; a.t_stride = P->t.cap; a.t_base = P->t_base; a.j0 = f->blocks;
    a.e_out = a.eu_out = a.du_out = nullptr; a.out_stride = 0;
    launch_impair(s, (int)(b1 - f->blocks), f->nchan, a);
    HIPCHK(hipGetLastError());
    ImpairReportArgs q;
    q.t = P->t.p[P->cur]; q.t_new = P->t.p[P->cur ^ 1]; q.t_stride = P->t.cap; q.t_base = P->t_base;
    q.t_base_new = b1 > RECORDS_KEPT ? b1 - RECORDS_KEPT : 0;
    q.j0 = f->blocks; q.j1 = b1; q.ja = a1 - 1; q.win = f->d_win; q.report = P->d_report;
    q.r = r.r; q.r_stride = r.r_stride; q.r_at = (long long)BLOCK * b1 - R_TAIL - r.r_base; q.r_tail = P->d_tail;
    launch_impair_report(s, f->nchan, q);
    HIPCHK(hipGetLastError());
    P->cur ^= 1; P->t_base = q.t_base_new;
    return 0;
}

extern "C" int nrsc5hip_fm_impair_enable(nrsc5hip_fm *f, const nrsc5hip_fm_impair_config *cfg)
{
    static_assert(RECORDS_KEPT == 2 * W + 1, "the windowed report reads 2 W + 1 block records");
    FM_ENABLE_CHECK(f, f->impair, "the impairment measurement");
    nrsc5hip_fm_impair_config c = {0.5, 0.05, 0.5};
    if (cfg) c = *cfg;
    if (!(c.explained_min >= 0.0 && c.explained_min <= 1.0)) FAIL(NRSC5HIP_EINVAL, "explained_min %g outside 0..1", c.explained_min);
    if (!(c.depth_min >= 0.0) || !std::isfinite(c.depth_min)) FAIL(NRSC5HIP_EINVAL, "depth_min %g: finite, at least 0", c.depth_min);
    if (!(c.rho_min >= 0.0 && c.rho_min <= 1.0)) FAIL(NRSC5HIP_EINVAL, "rho_min %g outside 0..1", c.rho_min);
    nrsc5::DeviceGuard guard(f->device);
    ImpairHost *P = new (std::nothrow) ImpairHost;
    if (!P) FAIL(NRSC5HIP_ENOMEM, "out of host memory");
    P->cfg = c;
    for (float v : hann_window()) P->wsum += (double)v;
    const std::vector<float> &hu = hu_table();
    const size_t K = (size_t)f->nchan;
#define ENABLE_CHK(expr) HIPCHK_OR(expr, delete P)
    ENABLE_CHK(P->t.alloc(RECORDS_KEPT + 256, f->nchan, NS));
    ENABLE_CHK(hipMalloc(&P->d_report, sizeof(double) * 2 * NS * K));
    ENABLE_CHK(hipMalloc(&P->d_tail, sizeof(float) * R_TAIL * K));
    ENABLE_CHK(hipMalloc(&P->d_hu, sizeof(float) * UT));
    ENABLE_CHK(hipMemcpy(P->d_hu, hu.data(), sizeof(float) * UT, hipMemcpyHostToDevice));
#undef ENABLE_CHK
    f->impair = P;
    int rc = impair_reset(f);
    if (!rc && !f->carrier) rc = nrsc5::carrier_enable(f);       // last: a failed enable leaves the object as it was
    if (rc) { f->impair = nullptr; delete P; }
    return rc;
}

extern "C" int nrsc5hip_fm_impair(nrsc5hip_fm *f, nrsc5hip_fm_impair_info *out)
{
    if (!f || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    FM_FEATURE_ENTER(f, impair, "the impairment measurement");
    ImpairHost *P = f->impair;
    std::vector<double> v(2 * NS * (size_t)f->nchan);
    HIPCHK(hipStreamSynchronize(f->stream));
    HIPCHK(hipMemcpy(v.data(), P->d_report, sizeof(double) * v.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < f->nchan; k++) {
        nrsc5hip_fm_impair_info &o = out[k];
        memset(&o, 0, sizeof(o));
        o.blocks = f->blocks; o.audio_blocks = f->audio_blocks;
        if (f->audio_blocks > 0) fill(o.windowed, &v[2 * NS * k], P->wsum);
        if (f->blocks > 0) fill(o.running, &v[2 * NS * k + NS], (double)f->blocks);
        figures(o.windowed, P->cfg); figures(o.running, P->cfg);
    }
    return 0;
}

extern "C" int nrsc5hip_fm_impair_taps(nrsc5hip_fm *f, float *hu)
{
    if (!f || !hu) FAIL(NRSC5HIP_EINVAL, "null argument");
    memcpy(hu, hu_table().data(), sizeof(float) * UT);
    return 0;
}

extern "C" int nrsc5hip_stage_fm_impair(nrsc5hip_fm *f, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *e_out, float *eu_out,
                                        float *du_out, double *sums_out)
{
    if (!f) FAIL(NRSC5HIP_EINVAL, "null demodulator");
    nrsc5::DeviceGuard guard(f->device);
    StageFront sf;
    const int rc = sf.open(f, dev_in, in_stride_elems, n_in, true, 1);
    if (rc) return rc;
    const long long m1 = sf.m1, b1 = sf.b1, mb = (long long)BLOCK * b1;
    if (b1 == 0) return 0;                                   // no complete block
    const size_t K = (size_t)f->nchan;
    const std::vector<float> &hu = hu_table();
    nrsc5::DevTmp e, eu, du, t, taps;
    HIPCHK(hipMalloc(&e.p, sizeof(float) * (size_t)mb * K));
    HIPCHK(hipMalloc(&eu.p, sizeof(float) * (size_t)mb * K));
    HIPCHK(hipMalloc(&du.p, sizeof(float) * (size_t)mb * K));
    HIPCHK(hipMalloc(&t.p, sizeof(double) * NS * (size_t)b1 * K));
    HIPCHK(hipMalloc(&taps.p, sizeof(float) * UT));
    HIPCHK(hipMemcpyAsync(taps.p, hu.data(), sizeof(float) * UT, hipMemcpyHostToDevice, f->stream));
    ImpairArgs q;
    q.r = sf.rf(); q.r_stride = m1; q.r_base = 0; q.r_tail = sf.rf();                            // the tail is not read: every m >= 0 is in r
    q.d = sf.df(); q.d_stride = m1; q.d_base = 0; q.hu = (const float *)taps.p;
    q.t = (double *)t.p; q.t_stride = b1; q.t_base = 0; q.j0 = 0;
    q.e_out = (float *)e.p; q.eu_out = (float *)eu.p; q.du_out = (float *)du.p; q.out_stride = mb;
    launch_impair(f->stream, (int)b1, f->nchan, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(f->stream));
    if (e_out) HIPCHK(hipMemcpy(e_out, e.p, sizeof(float) * (size_t)mb * K, hipMemcpyDeviceToHost));
    if (eu_out) HIPCHK(hipMemcpy(eu_out, eu.p, sizeof(float) * (size_t)mb * K, hipMemcpyDeviceToHost));
    if (du_out) HIPCHK(hipMemcpy(du_out, du.p, sizeof(float) * (size_t)mb * K, hipMemcpyDeviceToHost));
    if (sums_out) HIPCHK(hipMemcpy(sums_out, t.p, sizeof(double) * NS * (size_t)b1 * K, hipMemcpyDeviceToHost));
    return 0;
}
