// Host side of libnrsc5hip: the engine object's lifecycle -- read-only tables, creation, destruction, stream resets -- with the
// library's error text and build fingerprint and the small utilities of the C ABI (include/nrsc5hip.h).  The block-step scheduler is
// engine_steps.hip, the fast streaming seam engine_seam.hip, the batch API and fetch paths engine_batch.hip, the test hooks engine_stage.hip.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <new>
#include "engine_internal.h"

// ONE block-step chain per engine.  Cutting the stream set into half-sets on two chain queues was built and measured in round 3
// (profiles/r03_chain_lanes.txt: 49 vs 38 ms per pass -- the chip is occupancy-bound inside k_mixfft, a second queue only splits
// the same slots) and in round 1 (stream groups on separate HIP streams: nothing gained); the scaffolding for it is gone.
static_assert(sizeof(nrsc5hip_record) == sizeof(BlockRecord), "record ABI mismatch");
static_assert(sizeof(BlockRecord) % 8 == 0, "record alignment");

static thread_local char g_err[512] = "";
extern "C" const char *nrsc5hip_last_error(void) { return g_err; }
// the one error buffer of the library: every host-side unit reaches it through these two (host_util.h)
void nrsc5::set_last_error(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }
int nrsc5::fail(int code, const char *fmt, ...)
{
    char m[sizeof(g_err)];                                     // an argument may be the previous text itself
    va_list ap; va_start(ap, fmt); vsnprintf(m, sizeof(m), fmt, ap); va_end(ap);
    set_last_error(m);
    return code;
}
#ifndef NRSC5HIP_SOURCE_SHA
#define NRSC5HIP_SOURCE_SHA "unknown"
#endif
// the fingerprint behind a marker, so that a build can be identified from the FILE (nrsc5_amd.engine.check_fresh reads the bytes:
// a library that is already mapped into the process keeps answering for the old build after the file has been replaced)
static const char g_source_sha_marker[] = "NRSC5HIP_SOURCE_SHA=" NRSC5HIP_SOURCE_SHA;
extern "C" const char *nrsc5hip_source_sha(void) { return g_source_sha_marker + 20; }

template <typename T> static int dev_upload(nrsc5hip_engine *e, const T **p, const std::vector<T> &v)
{
    T *d; int rc = dev_alloc(e, &d, v.size()); if (rc) return rc;
    HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *p = d;
    return 0;
}

// ---- read-only tables --------------------------------------------------------------------------
static int build_tables(nrsc5hip_engine *e)
{
    static const int8_t PM_V[20] = { 10, 2, 18, 6, 14, 8, 16, 0, 12, 4, 11, 3, 19, 7, 15, 9, 17, 1, 13, 5 };   // decode.c:34-37
    // interleaver II for PIDS (decode.c:324-342 with b=200, I0=365440): index inside block bc
    std::vector<uint16_t> pids(16 * PIDS_CODED);
    for (unsigned bc = 0; bc < 16; bc++)
        for (unsigned n = 0; n < (unsigned)PIDS_CODED; n++) {
            const unsigned i = bc * PIDS_CODED + n, part = PM_V[i % 20];
            const unsigned k = ((i / 20) % (PIDS_CODED / 20)) + P1_CODED / (20 * 16);
            const unsigned row = (11 * k) % 32, col = (11 * k + k / (32 * 9)) % 36;
            pids[i] = (uint16_t)(row * 720 + part * 36 + col);
        }
    // descrambler stream (decode.c:279-294), packed LSB-first
    std::vector<uint32_t> scr(P1_WORDS, 0), scr_pids(3, 0);
    {
        unsigned val = 0x3ff;
        for (int i = 0; i < P1_LEN; i++) {
            const unsigned bit = ((val >> 9) ^ val) & 1;
            val |= bit << 11; val >>= 1;
            scr[i >> 5] |= bit << (i & 31);
            if (i < PIDS_LEN) scr_pids[i >> 5] |= bit << (i & 31);
        }
    }
    std::vector<float2> tw(FFT_N);
    for (int k = 0; k < FFT_N; k++) {
        const double a = -2.0 * M_PI * k / FFT_N;
        tw[k].x = (float)cos(a); tw[k].y = (float)sin(a);
    }
    std::vector<float> shape(SYM_N);                           // acquire.c:322-331
    for (int i = 0; i < SYM_N; i++) {
        if (i < CP_N) shape[i] = sinf(M_PI / 2 * i / CP_N);
        else if (i < FFT_N) shape[i] = 1;
        else shape[i] = cosf(M_PI / 2 * (i - FFT_N) / CP_N);
    }
    // Q15 taps: (int16)(tap * 32767.0f) as firdecim_q15_create does (firdecim_q15.c:37-42)
    static const float hb_taps[4] = { 0.6062333583831787f, -0.13481467962265015f, 0.032919470220804214f, -0.00410953676328063f };   // input.c:35-40
    static const float acq_taps[32] = {                        // acquire.c:28-61
        -0.000685643230099231f, 0.005636964458972216f, 0.009015781804919243f, -0.015486305579543114f,
        -0.035108357667922974f, 0.017446253448724747f, 0.08155813068151474f, 0.007995186373591423f,
        -0.13311293721199036f, -0.0727422907948494f, 0.15914097428321838f, 0.16498781740665436f,
        -0.1324498951435089f, -0.2484012246131897f, 0.051773931831121445f, 0.2821577787399292f,
        0.051773931831121445f, -0.2484012246131897f, -0.1324498951435089f, 0.16498781740665436f,
        0.15914097428321838f, -0.0727422907948494f, -0.13311293721199036f, 0.007995186373591423f,
        0.08155813068151474f, 0.017446253448724747f, -0.035108357667922974f, -0.015486305579543114f,
        0.009015781804919243f, 0.005636964458972216f, -0.000685643230099231f, 0.0f };
    std::vector<int16_t> hbq(4), acq(17, 0);
    for (int i = 0; i < 4; i++) hbq[i] = (int16_t)(hb_taps[3 - i] * 32767.0f);
    for (int i = 1; i <= 16; i++) acq[i] = (int16_t)(acq_taps[31 - i] * 32767.0f);

    int rc;
    if ((rc = dev_upload(e, &e->tb.pids_gather, pids))) return rc;
    {
        // MP1 equaliser: every data cell's operands, so that k_sync neither divides nor takes remainders per cell
        const int ncell = 2 * PM_PART * NSYM * 18;
        std::vector<uint32_t> cell(ncell);
        std::vector<uint16_t> outp(ncell);
        for (int c = 0; c < ncell; c++) {
            const int k = 1 + c % 18, n = (c / 18) % NSYM, part = (c / (18 * NSYM)) % PM_PART, side = c / (18 * NSYM * PM_PART);
            const int r_lo = side ? 2 * (part + 1) + 1 : 2 * part, r_hi = side ? 2 * part + 1 : 2 * (part + 1);
            const int ref_lo_bin = (r_lo & 1) ? UB1 - PW * (r_lo >> 1) : LB0 + PW * (r_lo >> 1);
            const int live = bin_to_live(ref_lo_bin + k);
            cell[c] = (uint32_t)live | (uint32_t)n << 10 | (uint32_t)r_lo << 15 | (uint32_t)r_hi << 20 | (uint32_t)k << 25 | (uint32_t)side << 30;
            outp[c] = (uint16_t)(n * 720 + (side ? 19 - part : part) * 36 + (k - 1) * 2);
        }
        if ((rc = dev_upload(e, &e->tb.eq_cell, cell))) return rc;
        if ((rc = dev_upload(e, &e->tb.eq_out, outp))) return rc;
    }
    {   // byte q of the 384-byte run of one k: q%6==5 is the erasure, else j = q - q/6, part = PM_V[j%20], block = (j/20 + 7 part) % 16
        std::vector<uint16_t> lut(384);
        for (int q = 0; q < 384; q++) {
            if (q % 6 == 5) { lut[q] = 0xffff; continue; }
            const int j = q - q / 6, part = PM_V[j % 20], block = (j / 20 + 7 * part) % 16;
            lut[q] = (uint16_t)(block * 720 + part * 36);
        }
        if ((rc = dev_upload(e, &e->tb.deint_lut, lut))) return rc;
    }
    if ((rc = dev_upload(e, &e->tb.scr_p1, scr))) return rc;
    if ((rc = dev_upload(e, &e->tb.scr_pids, scr_pids))) return rc;
    if ((rc = dev_upload(e, &e->tb.twiddle, tw))) return rc;
    {   // k_mixfft's first exchange: work-item r multiplies its k1-th output by W2048^(k1 r) -- from the plain table a gather with stride
        // k1 (up to 28 cache lines per wave and load), from this copy 256 consecutive entries per k1
        std::vector<float2> twa(7 * 256);
        for (int k1 = 1; k1 < 8; k1++) for (int r = 0; r < 256; r++) twa[(k1 - 1) * 256 + r] = tw[(k1 * r) & 2047];
        if ((rc = dev_upload(e, &e->tb.twiddle_a, twa))) return rc;
    }
    if ((rc = dev_upload(e, &e->tb.shape, shape))) return rc;
    if ((rc = dev_upload(e, &e->tb.hb_q15, hbq))) return rc;
    if ((rc = dev_upload(e, &e->tb.acq_q15, acq))) return rc;
    for (int wide = 0; wide < 2; wide++) {
        // interleaver IV (decode.c:344-376) is convolutional: position i of a block pair reads what was written
        // delay[i] positions earlier (1..N).  Same arithmetic as the reference's loop, for the first pair of a cycle.
        const unsigned L = wide ? 4608 : 2304, J = wide ? 4 : 2, C = 36, M = wide ? 2 : 4, N = 32 * L;
        const unsigned bk_bits = 32 * C, bk_adj = 32 * C - 1;
        std::vector<uint32_t> delay(2 * L);
        unsigned taken[4] = { 0, 0, 0, 0 };
        for (unsigned g = 0; g < 2 * L; g++) {
            const unsigned part = ((g + 2 * (M / 4)) / M) % J;
            const unsigned pti = taken[part]++;
            const unsigned block = (pti + (part * 7) - (bk_adj * (pti / bk_bits))) % 32;
            const unsigned row = ((11 * pti) % bk_bits) / C, col = (pti * 11) % C;
            const unsigned rp = (block * 32 + row) * (J * C) + part * C + col;
            const unsigned d = (g + N - rp) % N;
            delay[g] = d ? d : N;
        }
        if ((rc = dev_upload(e, wide ? &e->tb.px_delay_wide : &e->tb.px_delay_narrow, delay))) return rc;
    }
    {   // interleaver_ma1 (decode.c:66-231) folded into one table per code word: for every depunctured trellis input, which
        // bit of which hard-symbol matrix it is (bit_map), whether it passes the 3-frame diversity delay line, or a
        // punctured zero.  Same arithmetic as the reference's loops, evaluated once.
        static const int src12[12] = { 3, 0, 0, 3, 3, 0, 1, 1, 2, 2, 2, 1 };      // position in a 12-bit group -> bl / ml / bu / mu (decode.c:26-30)
        static const int j12[12] = { 2, 1, 0, 1, 0, 2, 1, 2, 1, 2, 0, 0 };
        static const int rank15[15] = { 0, -1, 1, 2, -1, 3, 4, -1, 5, 6, 7, 8, 9, 10, 11 };   // E1 puncture {1,0,1,1,0,1,1,0,1,1,1,1,1,1,1}
        auto cell_of = [](int b, int k) { const int col = (9 * k) % 25, row = (11 * col + 16 * (k / 25) + 11 * (k / 50)) % 32; return 25 * (b * 32 + row) + col; };
        // (the delay-line cell of a delayed input is keyed by the input's own index -- DevBuffers::am_q -- so the reference's queue /
        // position arguments only document which line it is)
        auto entry = [](int cell, int bit, int matrix, int delayed, int /*queue*/, int /*n*/) {
            return (uint32_t)((unsigned)cell | ((unsigned)bit << 13) | ((unsigned)matrix << 16) | (delayed ? AMT_DELAYED : 0u)); };
        std::vector<uint32_t> t1(AM_VIT), t3b(AM_VIT), t3a(3 * AM_P3_LEN_MA1);
        for (int i = 0; i < AM_VIT; i++) {
            const int rk = rank15[i % 15];
            if (rk < 0) { t1[i] = AMT_PUNCT; t3b[i] = t1[i]; continue; }
            const int o = (i / 15) * 12 + rk, g = o / 12, pos = o % 12, n = g * 3 + j12[pos];
            switch (src12[pos]) {       // matrices: 0 pl, 1 pu, 2 s, 3 t
            case 0: t1[i] = entry(cell_of(n / 2250, (n + n / 750 + 1) % 750), n % 3, 0, 0, 0, 0);                 // bl
                    t3b[i] = entry(cell_of((3 * n + 3) % 8, (n + n / 3000 + 3) % 750), n % 3, 3, 0, 0, 0); break;   // ebl
            case 1: t1[i] = entry(cell_of((3 * n + 3) % 8, (n + n / 3000 + 3) % 750), 3 + n % 3, 0, 1, 0, n);      // ml
                    t3b[i] = entry(cell_of((3 * n + 3) % 8, (n + n / 3000 + 3) % 750), 3 + n % 3, 3, 1, 2, n); break;   // eml
            case 2: t1[i] = entry(cell_of(n / 2250, (n + n / 750) % 750), n % 3, 1, 0, 0, 0);                     // bu
                    t3b[i] = entry(cell_of((3 * n) % 8, (n + n / 3000 + 2) % 750), n % 3, 2, 0, 0, 0); break;     // ebu
            default: t1[i] = entry(cell_of((3 * n) % 8, (n + n / 3000 + 2) % 750), 3 + n % 3, 1, 1, 1, n);         // mu
                    t3b[i] = entry(cell_of((3 * n) % 8, (n + n / 3000 + 2) % 750), 3 + n % 3, 2, 1, 3, n); break;  // emu
            }
        }
        for (int i = 0; i < 3 * AM_P3_LEN_MA1; i++) {             // E2 puncture {1,0,1,1,0,0}; 6-bit groups: el {0,1}, eu {2,3,5,4}
            const int r6 = i % 6;
            if (!(r6 == 0 || r6 == 2 || r6 == 3)) { t3a[i] = AMT_PUNCT; continue; }
            const int o = (i / 6) * 3 + (r6 == 0 ? 0 : r6 - 1), g = o / 6, pos = o % 6;
            if (pos < 2) { const int n = g * 2 + pos; t3a[i] = entry(cell_of((3 * n + n / 3000) % 8, (n + n / 6000) % 750), n % 2, 3, 0, 0, 0); }
            else {
                const int j = pos == 2 ? 0 : pos == 3 ? 1 : pos == 5 ? 2 : 3, n = g * 4 + j;
                t3a[i] = entry(cell_of((3 * n + n / 3000 + 2 * (n / 12000)) % 8, (n + n / 6000) % 750), n % 4, 2, 0, 0, 0);
            }
        }
        if ((rc = dev_upload(e, &e->tb.am_deint_p1, t1))) return rc;
        if ((rc = dev_upload(e, &e->tb.am_deint_p3_ma3, t3b))) return rc;
        if ((rc = dev_upload(e, &e->tb.am_deint_p3_ma1, t3a))) return rc;
    }
    {   // AM tables: acquisition FIR (acquire.c:63-96), pulse shape (acquire.c:333-342), 256-point twiddles
        static const float am_taps[32] = {
            -0.00038464731187559664f, -0.00021618751634377986f, 0.0026779419276863337f, -0.00029802651260979474f,
            -0.0012626448879018426f, -0.0013182522961869836f, -0.012252614833414555f, 0.015980124473571777f,
            0.037112727761268616f, -0.05451361835002899f, -0.05804193392395973f, 0.11320608854293823f,
            0.055298302322626114f, -0.16878043115139008f, -0.022917453199625015f, 0.19178225100040436f,
            -0.022917453199625015f, -0.16878043115139008f, 0.055298302322626114f, 0.11320608854293823f,
            -0.05804193392395973f, -0.05451361835002899f, 0.037112727761268616f, 0.015980124473571777f,
            -0.012252614833414555f, -0.0013182522961869836f, -0.0012626448879018426f, -0.00029802651260979474f,
            0.0026779419276863337f, -0.00021618751634377986f, -0.00038464731187559664f, 0.0f };
        std::vector<int16_t> amq(17, 0);
        for (int i = 1; i <= 16; i++) amq[i] = (int16_t)(am_taps[31 - i] * 32767.0f);
        std::vector<float> ashape(AM_SYM);
        for (int i = 0; i < AM_SYM; i++) {
            if (i < AM_CP) ashape[i] = sinf(M_PI / 2 * i / AM_CP);
            else if (i < AM_FFT) ashape[i] = 1;
            else ashape[i] = cosf(M_PI / 2 * (i - AM_FFT) / AM_CP);
        }
        std::vector<float2> atw(AM_FFT);
        for (int k = 0; k < AM_FFT; k++) { const double a = -2.0 * M_PI * k / AM_FFT; atw[k].x = (float)cos(a); atw[k].y = (float)sin(a); }
        if ((rc = dev_upload(e, &e->tb.am_acq_q15, amq))) return rc;
        if ((rc = dev_upload(e, &e->tb.am_shape, ashape))) return rc;
        if ((rc = dev_upload(e, &e->tb.am_twiddle, atw))) return rc;
    }
    return 0;
}

static void init_state(StreamState &st, int mode = MODE_FM)
{
    memset(&st, 0, sizeof(st));
    st.psmi = 1;                                               // sync_reset (sync.c:821)
    st.sync_state = SYNC_NONE;
    st.mode = mode;
    st.nco_re = 1.0f; st.nco_im = 0.0f; st.nco_exact = 1;     // acquire_reset: phase = 1 (acquire.c:296) -- from here on the float state can be kept bit for bit
}

static void init_am_state(AmStream &am)
{
    memset(&am, 0, sizeof(am));
    am.pli = am.hppi = am.aabi = am.rdbi = -1;                 // sync_reset (sync.c:822-825)
    am.am_diversity_wait = 4;                                  // decode_reset (decode.c:568)
    am.dec_bc = -1;
}

extern "C" int nrsc5hip_engine_create(const nrsc5hip_config *cfg, nrsc5hip_engine **out)
{
    if (!cfg || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->max_streams < 1 || cfg->q15_capacity < 2 * WIN_N || cfg->record_capacity < 64 || cfg->p1_slots < 2)
        FAIL(NRSC5HIP_EINVAL, "bad config (max_streams>=1, q15_capacity>=%d, record_capacity>=64, p1_slots>=2)", 2 * WIN_N);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) FAIL(NRSC5HIP_EINVAL, "device %d out of range (%d devices)", cfg->device, ndev);
    DeviceGuard guard(cfg->device);                            // the caller's current device is restored on return
    nrsc5hip_engine *e = new (std::nothrow) nrsc5hip_engine();
    if (!e) FAIL(NRSC5HIP_ENOMEM, "out of host memory");
    e->cfg = *cfg;
    const size_t S = cfg->max_streams;
    if (cfg->p1_async) {
        // the window pipeline drives 1 chain + 3 decode streams (+ the caller's): with the HIP runtime's default of 4 hardware
        // queues they share queues and the decode / chain overlap is lost silently
        const char *q = getenv("GPU_MAX_HW_QUEUES");
        static std::atomic<bool> warned{false};                // engines of one process share nothing else; this is a once-per-process notice
        if ((!q || atoi(q) < 8) && !warned.exchange(true)) {
            fprintf(stderr, "libnrsc5hip: warning: p1_async engine with GPU_MAX_HW_QUEUES=%s (< 8): decode streams will share hardware queues with "
                            "the block-step chain; export GPU_MAX_HW_QUEUES=8 before the HIP runtime initialises\n", q ? q : "unset (default 4)");
        }
    }
    int rc = 0;
    do {
        {
            // decode streams in use; nrsc5hip_debug_tune changes them.  FM: ONE since round 5 (three in rounds 2 - 4, profiles/r02_naux.txt): with the segmented forward pass
            // and the single-path traceback a window's decode (~1.6 ms) fits the 16 block steps of the next window (~1.7 ms) on one queue, and with two or three the
            // forward pass of one window overlaps the traceback of another -- the k_sync launch that meets both lasts 370 - 790 us instead of 37 (one per window; tools/gpu_trace_sync.sh,
            // profiles/r05_trace_sync_decode_streams.txt): 30.1 -> 29.2 ms per pass.  AM: three, with four segment waves per P3 frame (round 5, on the
            // rewritten block step: 70.4 ms with two streams x eight segments, 67.5 with three x eight, 65.7 with three x four, 91.3 with one: the K=9 decodes are ~80 ms of kernel time per pass)
            e->naux = 1; e->naux_am = 3;
            e->verdict_lag = 0; e->fwd_segments = 0; e->fwd_warm = 2; e->mixfft_syms = 1; e->sync_lanes = 0; e->flow_min = 0; e->tb_walk = 1; e->fuse_seam_prepare = 1; e->fold_report = 1;      // measured: profiles/r04_mixfft_persistent.txt
            e->am_segments = 4; e->am_warm = K9_WARM; e->am_runin = K9_TB_RUNIN;
        }
        {
            // (queue priorities -- chain stream high, decode streams low -- were measured: nothing for the batch, +15 % per block for
            // a lone stream, profiles/r02_ab_prio_demod.txt)
            if (hipStreamCreate(&e->main) != hipSuccess) rc = NRSC5HIP_EHIP;
            for (int k = 0; k < NAUX && !rc; k++) if (hipStreamCreate(&e->aux[k]) != hipSuccess) rc = NRSC5HIP_EHIP;
            for (int k = 0; k < NWIN && !rc; k++) {
                if (hipEventCreate(&e->ev_window[k]) != hipSuccess || hipEventCreate(&e->ev_decoded[k]) != hipSuccess) rc = NRSC5HIP_EHIP;
                e->decoded_pending[k] = false;
            }
            e->acq_needed = true; e->px_needed = true; e->set_sig = 0; e->step_count = 0; e->am_step_count = 0;
            for (int k = 0; k < NAUX; k++) e->lane_parity[k] = -1;
            e->thin = false;
            for (int k = 0; k < NWIN; k++) e->am_decoded_pending[k] = false;
            if (!rc && hipHostMalloc((void **)&e->counters_host, 4 * sizeof(int), hipHostMallocDefault) != hipSuccess) rc = NRSC5HIP_ENOMEM;
        }
        if (rc) { snprintf(g_err, sizeof(g_err), "stream/event creation failed"); break; }
        // K1 of the copying batch path runs ahead of the block steps on this stream (confining it to a slice of the CUs
        // with hipExtStreamCreateWithCUMask was measured: no gain, profiles/r02_k1cus.txt -- it is the HBM traffic itself that
        // slows the latency-bound step kernels; the zero-copy batch path has no K1 at all)
        if (hipStreamCreate(&e->dec_stream) != hipSuccess) { rc = NRSC5HIP_EHIP; snprintf(g_err, sizeof(g_err), "hipStreamCreate failed"); break; }
        e->dec_chunk = 0; e->chunk_nbytes_dev = nullptr; e->chunk_cap = 0;
        if ((rc = build_tables(e))) break;
        DevBuffers &db = e->db;
        db.q15_cap = cfg->q15_capacity; db.p1_slots = cfg->p1_slots; db.rec_cap = cfg->record_capacity;
        if ((rc = dev_alloc(e, &db.state, S))) break;
        db.ckpt = nullptr;
        if (cfg->p1_async && cfg->l2_feedback) {
            if (cfg->record_capacity < 2 * NWIN * 16) { rc = NRSC5HIP_EINVAL; snprintf(g_err, sizeof(g_err), "p1_async with l2_feedback needs record_capacity >= %d (speculated blocks keep their records)", 2 * NWIN * 16); break; }
            if ((rc = dev_alloc(e, &db.ckpt, S * NWIN))) break;
        }
        if ((rc = dev_alloc(e, &db.q15, S * (size_t)db.q15_cap))) break;
        db.acq_win = nullptr;
        if ((cfg->batch_zero_copy || !cfg->p1_async) && (rc = dev_alloc(e, &db.acq_win, S * WIN_N))) break;   // (fast-seam engines: the host-resident capture reads in place too)
        if ((rc = dev_alloc(e, &db.acq_filt, S * WIN_N))) break;
        if ((rc = dev_alloc(e, &db.acq_list, S + 1))) break;
        if ((rc = dev_alloc(e, &db.acq_sums, S * SYM_N))) break;
        if ((rc = dev_alloc(e, &db.bins, S * NSYM * LIVE_N))) break;
        // the reference's oscillator sample by sample for blocks in exact mode (553 KB per stream; k_nco_exact -> k_mixfft)
        if ((rc = dev_alloc(e, &db.nco_tab, S * NSYM * SYM_N))) break;
        if ((rc = dev_alloc(e, &db.cfo_snap, S * LIVE_N * (PM_PART + 1)))) break;
        if ((rc = dev_alloc(e, &db.cfo_phase, S * NSYM * LIVE_N))) break;     // 68 KB per stream: phases[][] of the exact CFO search's visit in progress
        e->flow_cap = flow_words((int)S); e->flow_bursts = e->flow_steps = 0;
        if ((rc = dev_alloc(e, &e->flow_dev, e->flow_cap))) break;
        if (hipHostMalloc((void **)&e->flow_err, 2 * sizeof(unsigned), hipHostMallocDefault) != hipSuccess) { rc = NRSC5HIP_ENOMEM; break; }
        e->flow_err[0] = e->flow_err[1] = 0;
        db.loop_exact = 1;                                     // the reference's own loop arithmetic in blocks that start un-synchronised (sync_body.h; NRSC5HIP_TUNE_LOOP_EXACT)
        // Default (round 6): a freshly reset stream's FIRST block -- the block its CFO search runs on -- advances the oscillator by the reference's own float recurrence
        // (k_nco_exact), every later block by the closed-form phasor with the recurrence's amplitude ramp.  Measured on the MI355X with the loop arithmetic of k_sync on the
        // reference's own operations (loop_exact below): 0 of 722 locks through the CFO search deviate in any field (768 / 768 streams strict), against 5 failing + 8 counted
        // streams with the closed form in that block (profiles/r06_nco_policy_decision.txt); cost 1.8 ms of a 30.4 ms pass.  (Round 5, with the fast loop arithmetic, had
        // seen no effect of the policy on the device and defaulted to NCO_CLOSED_FORM: both halves are needed.)  nrsc5hip_debug_tune(NRSC5HIP_TUNE_NCO_EXACT) changes it.
        db.nco_policy = NCO_EXACT_FIRST_BLOCK;
        if ((rc = dev_alloc(e, &db.pm, S * NPM * PM_FRAME))) break;
        db.nstreams_alloc = (int)S;
        if ((rc = dev_alloc(e, &db.coded, (size_t)(cfg->p1_async ? NAUX : 1) * S * P1_LEN))) break;
        if ((rc = dev_alloc(e, &db.dec, (size_t)(cfg->p1_async ? NAUX : 1) * S * (size_t)(2 * (P1_LEN + 64))))) break;
        if ((rc = dev_alloc(e, &db.tbmap, (size_t)(cfg->p1_async ? NAUX : 1) * S * (size_t)(P1_LEN / 64 + 1) * 64))) break;
        if ((rc = dev_alloc(e, &db.fwd_meta, (size_t)(cfg->p1_async ? NAUX : 1) * S * (size_t)(VIT3_GMAX * VIT3_META)))) break;
        if ((rc = dev_alloc(e, &db.fwd_stats, 4))) break;
        if (hipMemset(db.fwd_stats, 0, 4 * sizeof(int)) != hipSuccess) { rc = NRSC5HIP_EHIP; break; }
        db.tb_stats = db.fwd_stats + 2;
        if ((rc = dev_alloc(e, &db.am_k9stats, 4))) break;
        if (hipMemset(db.am_k9stats, 0, 4 * sizeof(unsigned)) != hipSuccess) { rc = NRSC5HIP_EHIP; break; }
        if ((rc = dev_alloc(e, &db.pids_stage, S * NWIN * 16 * 3 * PIDS_LEN))) break;
        if ((rc = dev_alloc(e, &db.pids_rec, S * NWIN * 16))) break;
        if (hipMemset(db.pids_rec, 0xff, S * NWIN * 16 * sizeof(int)) != hipSuccess) { rc = NRSC5HIP_EHIP; break; }
        if ((rc = dev_alloc(e, &db.p1_ring, S * db.p1_slots * P1_WORDS))) break;
        db.p1_mirror = nullptr;
        if ((rc = dev_alloc(e, &db.records, S * db.rec_cap))) break;
        if ((rc = dev_alloc(e, &db.counters, 4))) break;
        {
            const size_t nax = cfg->p1_async ? NAUX : 1;
            db.px_slots = 8 * cfg->p1_slots;
            if ((rc = dev_alloc(e, &db.px_mem, S * 2 * PX_MEM))) break;
            if ((rc = dev_alloc(e, &db.px_pair, S * 4 * PX_MAX))) break;
            if ((rc = dev_alloc(e, &db.px_stage, S * NWIN * 16 * (size_t)PX_DEPUNCT))) break;
            if ((rc = dev_alloc(e, &db.px_job, S * NWIN * 16))) break;
            if ((rc = dev_alloc(e, &db.px_dec, nax * S * 16 * (size_t)(PX_MAX + 64)))) break;
            if ((rc = dev_alloc(e, &db.px_ring, S * (size_t)db.px_slots * 2 * PX_WORDS))) break;
            if (hipMemset(db.px_mem, 0, S * 2 * PX_MEM) != hipSuccess || hipMemset(db.px_pair, 0, S * 4 * PX_MAX) != hipSuccess ||
                hipMemset(db.px_job, 0xff, S * NWIN * 16 * sizeof(PxJob)) != hipSuccess) { rc = NRSC5HIP_EHIP; snprintf(g_err, sizeof(g_err), "PX state init failed"); break; }
        }
        db.l2_ring = nullptr; db.l2_px_ring = nullptr; db.l2_am_ring = nullptr;
        if (cfg->l2_index) {
            if ((rc = dev_alloc(e, &db.l2_ring, S * (size_t)cfg->p1_slots))) break;
            if (hipMemset(db.l2_ring, 0, S * (size_t)cfg->p1_slots * sizeof(nrsc5hip_l2_frame)) != hipSuccess) { rc = NRSC5HIP_EHIP; break; }
            // ... and of every P3 / P4 frame slot, and (AM engines) of the nine frames of every AM L1 frame slot
            const size_t npx = S * (size_t)db.px_slots * 2, nam = cfg->am_enable ? S * (size_t)cfg->p1_slots * 9 : 0;
            if ((rc = dev_alloc(e, &db.l2_px_ring, npx))) break;
            if (hipMemset(db.l2_px_ring, 0, npx * sizeof(nrsc5hip_l2_frame)) != hipSuccess) { rc = NRSC5HIP_EHIP; break; }
            if (nam) {
                if ((rc = dev_alloc(e, &db.l2_am_ring, nam))) break;
                if (hipMemset(db.l2_am_ring, 0, nam * sizeof(nrsc5hip_l2_frame)) != hipSuccess) { rc = NRSC5HIP_EHIP; break; }
            }
        }
        db.am = nullptr; db.am_sym = nullptr; db.am_q = nullptr; db.am_vit = nullptr; db.am_dec = nullptr; db.am_k9meta = nullptr; db.am_job = nullptr; db.am_ckpt = nullptr; db.am_ber = nullptr; db.am_pids_stage = nullptr; db.am_pids_rec = nullptr; db.am_nvit = 1;
        if (cfg->am_enable) {
            if ((rc = dev_alloc(e, &db.am, S))) break;
            if ((rc = dev_alloc(e, &db.am_sym, S * 4 * AM_SYMS))) break;
            if ((rc = dev_alloc(e, &db.am_q, S * 3 * 2 * (size_t)AM_VIT))) break;
            db.am_nvit = cfg->p1_async ? NWIN : 1;
            const size_t ndec = cfg->p1_async ? NAUX : 1;
            if ((rc = dev_alloc(e, &db.am_vit, S * db.am_nvit * 2 * AM_VIT))) break;
            if ((rc = dev_alloc(e, &db.am_dec, ndec * S * (size_t)(8 * AM_DEC_P1 + AM_DEC_P3)))) break;
            if (cfg->p1_async && (rc = dev_alloc(e, &db.am_k9meta, ndec * S))) break;
            if ((rc = dev_alloc(e, &db.am_job, S * NWIN))) break;
            if ((rc = dev_alloc(e, &db.am_ber, S * (size_t)cfg->p1_slots))) break;
            if (cfg->p1_async && cfg->l2_feedback && (rc = dev_alloc(e, &db.am_ckpt, S * NWIN * 8))) break;      // replay checkpoints, one per delivered P1 PDU
            if ((rc = dev_alloc(e, &db.am_pids_stage, S * NWIN * 8 * (size_t)(3 * PIDS_LEN)))) break;
            if ((rc = dev_alloc(e, &db.am_pids_rec, S * NWIN * 8))) break;
            if (hipMemset(db.am_pids_rec, 0xff, S * NWIN * 8 * sizeof(int)) != hipSuccess) { rc = NRSC5HIP_EHIP; break; }
            if (hipMemset(db.am_job, 0, S * NWIN * sizeof(AmJob)) != hipSuccess || hipMemset(db.am_ber, 0, S * (size_t)cfg->p1_slots * sizeof(float)) != hipSuccess) { rc = NRSC5HIP_EHIP; break; }
            std::vector<AmStream> ainit(S);
            for (size_t k = 0; k < S; k++) init_am_state(ainit[k]);
            if (hipMemcpy(db.am, ainit.data(), S * sizeof(AmStream), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemset(db.am_q, 0, S * 3 * 2 * (size_t)AM_VIT) != hipSuccess || hipMemset(db.am_vit, 0, S * db.am_nvit * 2 * AM_VIT) != hipSuccess ||
                hipMemset(db.am_sym, 0, S * 4 * AM_SYMS) != hipSuccess) { rc = NRSC5HIP_EHIP; snprintf(g_err, sizeof(g_err), "AM state init failed"); break; }
        }
        db.sync_phase_cycles = nullptr;        // nrsc5hip_debug_tune(NRSC5HIP_TUNE_SYNC_PHASES) turns the instrumentation on
        e->stage_bytes = 4u << 20; e->stage_ring_bytes = 1u << 20;
        if ((rc = dev_alloc(e, &e->stage_dev, e->stage_bytes))) break;
        if (!cfg->p1_async) {
            for (int k = 0; k < nrsc5hip_engine::NSTAGE && !rc; k++) {
                if ((rc = dev_alloc(e, &e->stage_dev2[k], e->stage_ring_bytes + 16))) break;
                void *sp = nullptr;
                if (hipHostMalloc((void **)&e->stage_pin[k], e->stage_ring_bytes + 16, hipHostMallocMapped) != hipSuccess ||
                    hipHostGetDevicePointer(&sp, e->stage_pin[k], 0) != hipSuccess ||
                    hipEventCreateWithFlags(&e->stage_ev[k], hipEventDisableTiming) != hipSuccess) { rc = NRSC5HIP_ENOMEM; snprintf(g_err, sizeof(g_err), "pinned staging allocation failed"); }
                e->stage_pin_dev[k] = (uint8_t *)sp;
                e->stage_busy[k] = false;
            }
            if (rc) break;
            if (S * (size_t)cfg->p1_slots <= 64) {
                // the fast seam's P1 frames reach the host by the traceback's own stores (k_p1_traceback writes the pinned mirror beside the
                // device ring): nrsc5hip_p1_frame_packed then copies 18 KB of host memory instead of synchronising and issuing a D2H copy
                const size_t nw = S * (size_t)cfg->p1_slots * P1_WORDS;
                void *mp = nullptr;
                if (hipHostMalloc((void **)&e->frames_host, nw * sizeof(uint32_t), hipHostMallocMapped) != hipSuccess ||
                    hipHostGetDevicePointer(&mp, e->frames_host, 0) != hipSuccess) { rc = NRSC5HIP_ENOMEM; snprintf(g_err, sizeof(g_err), "pinned frame mirror allocation failed"); break; }
                memset(e->frames_host, 0, nw * sizeof(uint32_t));
                db.p1_mirror = (uint32_t *)mp;
            }
            // The ingest stream gets a queue priority of its own: HIP streams of one priority share a small pool of hardware queues, and
            // whether `ingest` and `main` landed on the same one -- which serialises the early chunks with the block step they are meant
            // to run beside -- depended on how many streams the process had created before (measured: the same drop-in build at 1110 x or
            // 820 x real time, from one process to the next).  Queues of different priorities are never shared.
            int prio_least = 0, prio_greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
            if (hipStreamCreateWithPriority(&e->ingest, hipStreamDefault, prio_greatest) != hipSuccess || hipEventCreateWithFlags(&e->ev_ingest, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&e->ev_main, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&e->ev_appended, hipEventDisableTiming) != hipSuccess) { rc = NRSC5HIP_EHIP; snprintf(g_err, sizeof(g_err), "ingest stream creation failed"); break; }
            e->ingest_dirty = false; e->main_stepped = false; e->main_appended = false; e->early_flush = 128u << 10;     // a block is 270 KB of cu8: 128 + 128 + a last chunk of ~14 KB
            if ((rc = dev_alloc(e, &e->decim_ticket, 1))) break;
            if (hipMemset(e->decim_ticket, 0, sizeof(unsigned)) != hipSuccess) { rc = NRSC5HIP_EHIP; break; }
            for (int k = 0; k < 2 && !rc; k++) {
                void *dp = nullptr;
                if (hipHostMalloc((void **)&e->report_host[k], sizeof(StreamReport), hipHostMallocMapped) != hipSuccess ||
                    hipHostGetDevicePointer(&dp, e->report_host[k], 0) != hipSuccess) { rc = NRSC5HIP_ENOMEM; snprintf(g_err, sizeof(g_err), "pinned report allocation failed"); break; }
                e->report_dev[k] = (StreamReport *)dp;
                memset(e->report_host[k], 0, sizeof(StreamReport));
            }
            if (rc) break;
        }
        e->hc_stream = -1; e->hc_abs0 = 0; e->hc_wr = 0; e->host_capture = false; e->hc_rebases = e->hc_attaches = e->hc_detaches = 0; e->reports_folded = 0;
        if (!cfg->p1_async) {
            e->hc_cap = 16u << 20;                             // 58 FM blocks between two rebases (~300 KB of host memmove each)
            void *hp = nullptr;
            if (hipHostMalloc((void **)&e->hc_pin, e->hc_cap, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&hp, e->hc_pin, 0) != hipSuccess) {
                rc = NRSC5HIP_ENOMEM; snprintf(g_err, sizeof(g_err), "pinned capture allocation failed"); break;
            }
            e->hc_dev = (uint8_t *)hp; e->host_capture = true;
        }
        e->hb_hist_host.assign(S, std::array<c16, 14>{});
        e->stage_slot = 0; e->staged_stream = -1; e->staged_bytes = 0; e->staged_q15 = 0; e->staged_cu8 = false;
        if ((rc = dev_alloc(e, &e->ids_dev, S))) break;
        if ((rc = dev_alloc(e, &e->nbytes_dev, S))) break;
        if ((rc = dev_alloc(e, &e->all_ids_dev, S))) break;
        if ((rc = dev_alloc(e, &e->trim_plan_dev, S))) break;
        std::vector<StreamState> init(S);
        std::vector<int> ident(S);
        for (size_t s = 0; s < S; s++) { init_state(init[s]); ident[s] = (int)s; }
        if (hipMemcpy(db.state, init.data(), S * sizeof(StreamState), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(e->all_ids_dev, ident.data(), S * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(db.records, 0, S * db.rec_cap * sizeof(BlockRecord)) != hipSuccess ||
            hipMemset(db.pm, 0, S * NPM * PM_FRAME) != hipSuccess) { rc = NRSC5HIP_EHIP; snprintf(g_err, sizeof(g_err), "state init copy failed"); break; }
        e->wr_host.assign(S, 0); e->base_host.assign(S, 0); e->drained.assign(S, 0);
        e->mode_host.assign(S, MODE_FM); e->raw_host.assign(S, 0); e->attached.assign(S, 0);
        e->rd_host.assign(S, 0); e->fetched.assign(S, 0); e->mirror_ok.assign(S, cfg->p1_async ? 0 : 1); e->pending.assign(S, {});
        e->pred_ok.assign(S, 0); e->pred_samperr.assign(S, 0); e->pred_bc.assign(S, 0); e->manual_step.assign(S, 0);
        e->inflight_stream = -1; e->report_seq = 0; e->inflight_rd_pred = -1; e->inflight_decoded = true; e->inflight_progress = false; e->inflight_seq = 0; e->ahead.valid = false;
        e->defer_wait = true; e->direct_decimate = true; e->counters_clean = false;
        e->prof_on = false; e->prof_only = -1;
        for (int k = 0; k < NRSC5HIP_PROF_CLASSES; k++) { e->prof_ms[k] = 0; e->prof_launches[k] = 0; }
    } while (0);
    if (rc) { nrsc5hip_engine_destroy(e); return rc; }
    *out = e;
    return NRSC5HIP_OK;
}

extern "C" void nrsc5hip_engine_destroy(nrsc5hip_engine *e)
{
    if (!e) return;
    DeviceGuard guard(e->cfg.device);
    (void)hipDeviceSynchronize();
    vit_scratch_free(e->vit_scratch);
    for (void *p : e->allocs) (void)hipFree(p);
    for (hipEvent_t ev : e->dec_events) (void)hipEventDestroy(ev);
    if (e->dec_stream) (void)hipStreamDestroy(e->dec_stream);
    if (e->flow_err) (void)hipHostFree(e->flow_err);
    if (e->rec_host) (void)hipHostFree(e->rec_host);
    if (e->frames_host) (void)hipHostFree(e->frames_host);
    if (e->nblocks_host) (void)hipHostFree(e->nblocks_host);
    for (int k = 0; k < nrsc5hip_engine::NSTAGE; k++) { if (e->stage_pin[k]) (void)hipHostFree(e->stage_pin[k]); if (e->stage_ev[k]) (void)hipEventDestroy(e->stage_ev[k]); }
    for (int k = 0; k < 2; k++) if (e->report_host[k]) (void)hipHostFree(e->report_host[k]);
    if (e->hc_pin) (void)hipHostFree(e->hc_pin);
    if (e->ingest) (void)hipStreamDestroy(e->ingest);
    if (e->ev_ingest) (void)hipEventDestroy(e->ev_ingest);
    if (e->ev_main) (void)hipEventDestroy(e->ev_main);
    if (e->ev_appended) (void)hipEventDestroy(e->ev_appended);
    for (auto &sp : e->prof_spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    for (hipEvent_t ev : e->prof_pool) (void)hipEventDestroy(ev);
    if (e->counters_host) (void)hipHostFree(e->counters_host);
    for (int k = 0; k < NWIN; k++) { if (e->ev_window[k]) (void)hipEventDestroy(e->ev_window[k]); if (e->ev_decoded[k]) (void)hipEventDestroy(e->ev_decoded[k]); }
    if (e->main) (void)hipStreamDestroy(e->main);
    for (int k = 0; k < NAUX; k++) if (e->aux[k]) (void)hipStreamDestroy(e->aux[k]);
    delete e;
}

extern "C" void *nrsc5hip_engine_hip_stream(nrsc5hip_engine *e) { return e ? (void *)e->main : nullptr; }

// nrsc5hip_hdc_feed (hdc_consumer.hip) checks its stream ids before it touches the consumer
int nrsc5_engine_max_streams(const nrsc5hip_engine *e) { return e ? e->cfg.max_streams : 0; }

// input_reset (input.c:126-138).  keep_windows: the reference's reset of a USED session -- firdecim_q15_reset rewinds the index of every FIR window
// and leaves its samples (firdecim_q15.c:53-56), so decim[0]'s first outputs and the acquisition filter's first 31 see what the last compaction of
// their windows left there (StaleWindows, nrsc5_dev.h).  Otherwise a fresh session (nrsc5_open_pipe: calloc'd windows).
static int reset_stream(nrsc5hip_engine *e, int stream, bool keep_windows)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (e->staged_stream == stream) {
        // samples not yet submitted die with the session -- but the reference's decimator has seen them (decimate_samples runs inside the push): when the
        // windows are kept they go through the decimator first (no block step: wr alone moves, and the reset below forgets it)
        if (keep_windows && e->staged_bytes && (rc = flush_staged(e))) return rc;
        e->staged_stream = -1; e->staged_bytes = 0; e->staged_q15 = 0;
    }
    // this engine's queues only (another session of the process keeps running)
    if (e->ingest) HIPCHK(hipStreamSynchronize(e->ingest));
    HIPCHK(hipStreamSynchronize(e->main));
    if (e->cfg.p1_async) { for (int k = 0; k < NAUX; k++) HIPCHK(hipStreamSynchronize(e->aux[k])); HIPCHK(hipStreamSynchronize(e->dec_stream)); }
    StreamState st; init_state(st, e->mode_host[stream]);
    const bool was_hc = e->hc_stream == stream;
    if (keep_windows && !e->cfg.batch_zero_copy) {             // (zero-copy engines: every attach is an independent recording, read in place with byte-valued history)
        HIPCHK(hipMemcpy(&st.stale, (const char *)(e->db.state + stream) + offsetof(StreamState, stale), sizeof(st.stale), hipMemcpyDeviceToHost));
        // sync_reset (sync.c:810-830) leaves sync_t.samperr, .angle and .bc alone.  The FM path overwrites all three in the block that locks, before anything reads
        // them; the AM path never writes .angle, so the first synchronised block of an AM session after an FM one turns by the FM session's last angle
        // (acquire.c:115-118) -- and the block records of the un-synchronised blocks in between show the old values
        HIPCHK(hipMemcpy(&st.samperr, (const char *)(e->db.state + stream) + offsetof(StreamState, samperr), sizeof(st.samperr), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&st.angle, (const char *)(e->db.state + stream) + offsetof(StreamState, angle), sizeof(st.angle), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&st.bc, (const char *)(e->db.state + stream) + offsetof(StreamState, bc), sizeof(st.bc), hipMemcpyDeviceToHost));
        // a stream that read the pinned capture never ran the streaming decimator: what decim[0]'s window holds after every byte pushed in that session is told from the capture
        if (was_hc) (void)hc_stale_hb(e, (e->hc_wr - nrsc5hip_engine::HC_PREFIX) / 2, st.stale.hb);
        st.stale.hb_pushed = 0; st.stale.fir_pushed[0] = 0; st.stale.fir_pushed[1] = 0;
        memcpy(st.hb_hist, st.stale.hb, sizeof(st.hb_hist));
        memcpy(st.fir_hist, st.stale.fir[st.mode == MODE_AM ? MODE_AM : MODE_FM], sizeof(st.fir_hist));
    }
    HIPCHK(hipMemcpy(e->db.state + stream, &st, sizeof(st), hipMemcpyHostToDevice));
    if (e->db.am) {
        AmStream am; init_am_state(am);
        memcpy(am.seed[0], st.stale.hb, sizeof(am.seed[0]));   // zeros unless the windows were kept
        memcpy(am.seed[1], st.stale.am_stage, sizeof(st.stale.am_stage));
        HIPCHK(hipMemcpy(e->db.am + stream, &am, sizeof(am), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(e->db.am_job + (size_t)stream * NWIN, 0, NWIN * sizeof(AmJob)));
        HIPCHK(hipMemset(e->db.am_pids_rec + (size_t)stream * NWIN * 8, 0xff, NWIN * 8 * sizeof(int)));
    }
    if (was_hc) e->hc_stream = -1;
    memcpy(e->hb_hist_host[stream].data(), st.hb_hist, sizeof(st.hb_hist));
    e->wr_host[stream] = 0; e->base_host[stream] = 0; e->drained[stream] = 0; e->raw_host[stream] = 0; e->attached[stream] = 0;
    e->rd_host[stream] = 0; e->fetched[stream] = 0; e->pending[stream].clear(); e->mirror_ok[stream] = e->cfg.p1_async ? 0 : 1;
    forget_prediction(e, stream);
    e->acq_needed = true; e->px_needed = true; e->set_sig = 0;
    return 0;
}

extern "C" int nrsc5hip_stream_reset(nrsc5hip_engine *e, int stream) { return reset_stream(e, stream, true); }
extern "C" int nrsc5hip_stream_fresh(nrsc5hip_engine *e, int stream) { return reset_stream(e, stream, false); }

// nrsc5_set_mode -> input_set_mode (input.c:158-162): switch the stream's waveform and reset it
extern "C" int nrsc5hip_stream_set_mode(nrsc5hip_engine *e, int stream, int mode)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (mode != NRSC5HIP_MODE_FM && mode != NRSC5HIP_MODE_AM) FAIL(NRSC5HIP_EINVAL, "unknown mode %d", mode);
    if (mode == NRSC5HIP_MODE_AM && !e->db.am) FAIL(NRSC5HIP_EINVAL, "engine was created without am_enable");
    if (mode == NRSC5HIP_MODE_AM && e->db.q15_cap < 2 * AM_WIN) FAIL(NRSC5HIP_EINVAL, "q15_capacity too small");
    if (e->staged_stream == stream && e->staged_bytes && (rc = flush_staged(e))) return rc;     // bytes pushed in the old mode pass through the old mode's decimator (reset_stream)
    e->mode_host[stream] = mode;
    return nrsc5hip_stream_reset(e, stream);
}

__global__ void k_force_none(DevBuffers db, int s) { db.state[s].sync_state = SYNC_NONE; }

extern "C" int nrsc5hip_force_resync(nrsc5hip_engine *e, int stream)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    hipLaunchKernelGGL(k_force_none, dim3(1), dim3(1), 0, e->main, e->db, stream);
    forget_prediction(e, stream);
    e->acq_needed = true; e->px_needed = true; e->set_sig = 0;
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- device helpers for C hosts that do not link the HIP runtime themselves (integration/batch_shard.c) ------------------------------
extern "C" int nrsc5hip_device_count(int *n)
{
    if (!n) FAIL(NRSC5HIP_EINVAL, "null argument");
    HIPCHK(hipGetDeviceCount(n));
    return 0;
}
extern "C" int nrsc5hip_device_upload(int device, const void *host, size_t nbytes, void **dev_out)
{
    if (!dev_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    *dev_out = nullptr;
    DeviceGuard guard(device);
    void *d = nullptr;
    if (hipMalloc(&d, nbytes ? nbytes : 1) != hipSuccess) FAIL(NRSC5HIP_ENOMEM, "hipMalloc(%zu bytes) on device %d failed", nbytes, device);
    if (host) { hipError_t err = hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice); if (err != hipSuccess) { (void)hipFree(d); FAIL(NRSC5HIP_EHIP, "upload failed: %s", hipGetErrorString(err)); } }
    *dev_out = d;
    return 0;
}
extern "C" int nrsc5hip_device_free(int device, void *dev)
{
    DeviceGuard guard(device);
    HIPCHK(hipFree(dev));
    return 0;
}

extern "C" int nrsc5hip_reset_all(nrsc5hip_engine *e)
{
    ON_ENGINE_DEVICE(e);
    if (!e) FAIL(NRSC5HIP_EINVAL, "null engine");
    HIPCHK(hipDeviceSynchronize());
    e->dec_chunk = 0;
    e->staged_stream = -1; e->staged_bytes = 0; e->staged_q15 = 0;
    e->hc_stream = -1; std::fill(e->hb_hist_host.begin(), e->hb_hist_host.end(), std::array<c16, 14>{});
    const size_t S = e->cfg.max_streams;
    std::vector<StreamState> init(S);
    for (size_t s = 0; s < S; s++) init_state(init[s], e->mode_host[s]);
    HIPCHK(hipMemcpy(e->db.state, init.data(), S * sizeof(StreamState), hipMemcpyHostToDevice));
    if (e->db.am) {
        std::vector<AmStream> ainit(S);
        for (size_t s = 0; s < S; s++) init_am_state(ainit[s]);
        HIPCHK(hipMemcpy(e->db.am, ainit.data(), S * sizeof(AmStream), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(e->db.am_job, 0, S * NWIN * sizeof(AmJob)));
        HIPCHK(hipMemset(e->db.am_pids_rec, 0xff, S * NWIN * 8 * sizeof(int)));
    }
    std::fill(e->raw_host.begin(), e->raw_host.end(), 0);
    std::fill(e->attached.begin(), e->attached.end(), 0);
    std::fill(e->wr_host.begin(), e->wr_host.end(), 0);
    std::fill(e->base_host.begin(), e->base_host.end(), 0);
    std::fill(e->drained.begin(), e->drained.end(), 0);
    std::fill(e->rd_host.begin(), e->rd_host.end(), 0);
    std::fill(e->fetched.begin(), e->fetched.end(), 0);
    std::fill(e->mirror_ok.begin(), e->mirror_ok.end(), (char)(e->cfg.p1_async ? 0 : 1));
    std::fill(e->pred_ok.begin(), e->pred_ok.end(), 0); e->counters_clean = false;
    for (auto &q : e->pending) q.clear();
    HIPCHK(hipMemset(e->db.pids_rec, 0xff, S * NWIN * 16 * sizeof(int)));
    HIPCHK(hipMemset(e->db.px_job, 0xff, S * NWIN * 16 * sizeof(PxJob)));
    e->acq_needed = true; e->px_needed = true; e->set_sig = 0; e->step_count = 0; e->am_step_count = 0;
    for (int k = 0; k < NWIN; k++) { e->am_decoded_pending[k] = false; e->decoded_pending[k] = false; }
    return 0;
}

void nrsc5::prof_collect(nrsc5hip_engine *e)
{
    // caller has synchronised both streams
    for (auto &sp : e->prof_spans) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) { e->prof_ms[sp.cls] += ms; e->prof_launches[sp.cls]++; }
        e->prof_pool.push_back(sp.a); e->prof_pool.push_back(sp.b);
    }
    e->prof_spans.clear();
}

extern "C" int nrsc5hip_profile(nrsc5hip_engine *e, int enable, double *total_ms, long long *launches)
{
    ON_ENGINE_DEVICE(e);
    if (!e) FAIL(NRSC5HIP_EINVAL, "null engine");
    HIPCHK(hipDeviceSynchronize());
    if (e->prof_on) prof_collect(e);
    for (int k = 0; k < NRSC5HIP_PROF_CLASSES; k++) {
        if (total_ms) total_ms[k] = e->prof_ms[k];
        if (launches) launches[k] = e->prof_launches[k];
        if (enable >= 0) { e->prof_ms[k] = 0; e->prof_launches[k] = 0; }
    }
    if (enable >= 0) { e->prof_on = enable != 0; e->prof_only = (enable & 0x100) ? (enable & 0xff) : -1; }
    return 0;
}

extern "C" int nrsc5hip_abi_version(void) { return NRSC5HIP_ABI_VERSION; }
