// Test hooks and micro-benchmarks: every nrsc5hip_stage_* and nrsc5hip_debug_* entry point (single kernels on caller data, peeks at
// device state, counters) and the tuning knobs (nrsc5hip_debug_tune).  Nothing here runs in a production pass.
#include <algorithm>
#include <cmath>
#include "engine_internal.h"

extern "C" void nrsc5hip_debug_seam_totals(double out[8], int reset)
{
    for (int k = 0; k < 8; k++) { if (out) out[k] = g_seam[k]; if (reset) g_seam[k] = 0; }
}
extern "C" void nrsc5hip_debug_seam_counts(double out[6], int reset)
{
    for (int k = 0; k < 6; k++) { if (out) out[k] = g_seam[8 + k]; if (reset) g_seam[8 + k] = 0; }
}

extern "C" int nrsc5hip_stage_l2_index(nrsc5hip_engine *e, const uint8_t *bits, int nbits, int nframes, nrsc5hip_l2_frame *out, uint8_t *pdu_bytes, long long stride)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !bits || !out || nbits < 1 || nframes < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    const int words = (nbits + 31) / 32;
    std::vector<uint32_t> w((size_t)words * nframes, 0u);
    for (int f = 0; f < nframes; f++)
        for (int i = 0; i < nbits; i++) w[(size_t)f * words + (i >> 5)] |= (uint32_t)(bits[(size_t)f * nbits + i] & 1u) << (i & 31);
    DevTmp tw;
    HIPCHK(hipMalloc(&tw.p, w.size() * sizeof(uint32_t)));
    uint32_t *dw = (uint32_t *)tw.p;
    HIPCHK(hipMemcpy(dw, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    std::vector<L2Job> dj((size_t)nframes);
    for (int f = 0; f < nframes; f++) dj[f] = L2Job{dw + (size_t)f * words, nbits, 0};
    return l2_run(e, dj, out, pdu_bytes, stride);
}

extern "C" int nrsc5hip_stage_first_header(nrsc5hip_engine *e, const uint8_t *bits, int nbits, int nframes, int threads, int *ok)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !bits || !ok || nframes < 1 || (nbits != P1_LEN && nbits != AM_P1_LEN) || threads < 64 || threads > 1024 || (threads & 63)) FAIL(NRSC5HIP_EINVAL, "bad argument");
    const int words = (nbits + 31) / 32;
    std::vector<uint32_t> w((size_t)nframes * words, 0u);
    for (int f = 0; f < nframes; f++)
        for (int i = 0; i < nbits; i++) if (bits[(size_t)f * nbits + i] & 1) w[(size_t)f * words + (i >> 5)] |= 1u << (i & 31);
    uint32_t *dw = nullptr; int *dok = nullptr;
    HIPCHK(hipMalloc((void **)&dw, w.size() * sizeof(uint32_t)));
    HIPCHK(hipMalloc((void **)&dok, (size_t)nframes * sizeof(int)));
    HIPCHK(hipMemcpy(dw, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    launch_stage_first_header(dw, words, nframes, nbits == AM_P1_LEN ? 1 : 0, threads, dok, e->main);
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(ok, dok, (size_t)nframes * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(dw); (void)hipFree(dok);
    return 0;
}

extern "C" int nrsc5hip_stage_viterbi_k9(nrsc5hip_engine *e, const int8_t *soft, int len, int nframes, const unsigned gens[3], uint8_t *bits)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !soft || !bits || !gens || len < 64 || nframes < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    int8_t *dsoft = nullptr; unsigned long long *ddec = nullptr; uint32_t *dout = nullptr;
    const int words = (len + 31) / 32;
    HIPCHK(hipMalloc((void **)&dsoft, (size_t)nframes * 3 * len));
    HIPCHK(hipMalloc((void **)&ddec, (size_t)nframes * 4 * (len + 64) * sizeof(unsigned long long)));
    HIPCHK(hipMalloc((void **)&dout, (size_t)nframes * words * sizeof(uint32_t)));
    HIPCHK(hipMemcpy(dsoft, soft, (size_t)nframes * 3 * len, hipMemcpyHostToDevice));
    K9Meta *dmeta = nullptr;                                   // segment waves (the window pipeline's form) unless tuned down to one
    if (e->am_segments > 1 && len > 80) HIPCHK(hipMalloc((void **)&dmeta, (size_t)nframes * sizeof(K9Meta)));
    launch_viterbi_k9_frames(dsoft, len, nframes, gens[0], gens[1], gens[2], ddec, dout, e->main, 3, dmeta, e->am_segments, e->am_warm, e->am_runin, e->db.am_k9stats);
    HIPCHK(hipStreamSynchronize(e->main));
    if (dmeta) (void)hipFree(dmeta);
    std::vector<uint32_t> w((size_t)nframes * words);
    HIPCHK(hipMemcpy(w.data(), dout, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int f = 0; f < nframes; f++) nrsc5hip_unpack_bits(w.data() + (size_t)f * words, len, bits + (size_t)f * len);
    (void)hipFree(dsoft); (void)hipFree(ddec); (void)hipFree(dout);
    return 0;
}

// ---- stage-level entry points ----------------------------------------------------------------------------------------
extern "C" int nrsc5hip_stage_halfband_fm_cu8(nrsc5hip_engine *e, const uint8_t *iq, uint32_t nbytes, int16_t *out)
{
    ON_ENGINE_DEVICE(e);
    // runs the production K1 kernel on stream 0 of a scratch state: requires a freshly reset stream 0
    int rc = check_stream(e, 0); if (rc) return rc;
    if (nbytes % 4 || nbytes > e->stage_bytes || nbytes / 4 > e->db.q15_cap) FAIL(NRSC5HIP_EINVAL, "bad length");
    if ((rc = nrsc5hip_stream_fresh(e, 0))) return rc;
    const int s = 0; const unsigned count = nbytes;
    HIPCHK(hipMemcpy(e->stage_dev, iq, nbytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->ids_dev, &s, sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->nbytes_dev, &count, sizeof(unsigned), hipMemcpyHostToDevice));
    launch_decimate_fm_cu8(e->tb, e->db, 1, e->ids_dev, e->stage_dev, 0, e->nbytes_dev, count, e->main);
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(out, e->db.q15, (size_t)(nbytes / 4) * sizeof(c16), hipMemcpyDeviceToHost));
    return nrsc5hip_stream_fresh(e, 0);
}

extern "C" int nrsc5hip_stage_fft2048(nrsc5hip_engine *e, const float *in, float *out, int n)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !in || !out || n < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    float2 *din = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)n * FFT_N * sizeof(float2);
    HIPCHK(hipMalloc((void **)&din, bytes));
    HIPCHK(hipMalloc((void **)&dout, bytes));
    HIPCHK(hipMemcpy(din, in, bytes, hipMemcpyHostToDevice));
    launch_fft2048(e->tb, din, dout, n, e->main, e->mixfft_syms);
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    (void)hipFree(din); (void)hipFree(dout);
    return 0;
}

extern "C" int nrsc5hip_stage_viterbi_k7(nrsc5hip_engine *e, const int8_t *soft, int len, int nframes, uint8_t *bits)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !soft || !bits || len < 64 || nframes < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    int8_t *dsoft = nullptr; unsigned long long *ddec = nullptr; uint32_t *dout = nullptr;
    const int words = (len + 31) / 32;
    HIPCHK(hipMalloc((void **)&dsoft, (size_t)nframes * 3 * len));
    HIPCHK(hipMalloc((void **)&ddec, (size_t)nframes * (len + 64) * sizeof(unsigned long long)));
    HIPCHK(hipMalloc((void **)&dout, (size_t)nframes * words * sizeof(uint32_t)));
    HIPCHK(hipMemcpy(dsoft, soft, (size_t)nframes * 3 * len, hipMemcpyHostToDevice));
    if (launch_viterbi_frames(e->vit_scratch, dsoft, len, nframes, ddec, dout, e->main, 3 | (e->tb_walk ? 0 : 16), e->fwd_segments > 0 ? e->fwd_segments : 16, e->db.fwd_stats, e->fwd_warm)) FAIL(NRSC5HIP_EINVAL, "frame length %d not supported or out of device memory", len);
    HIPCHK(hipStreamSynchronize(e->main));
    std::vector<uint32_t> w((size_t)nframes * words);
    HIPCHK(hipMemcpy(w.data(), dout, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int f = 0; f < nframes; f++) nrsc5hip_unpack_bits(w.data() + (size_t)f * words, len, bits + (size_t)f * len);
    (void)hipFree(dsoft); (void)hipFree(ddec); (void)hipFree(dout);
    return 0;
}

extern "C" int nrsc5hip_debug_fetch(nrsc5hip_engine *e, int stream, int8_t *pm, float *bins)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    if (pm) {
        int slot = 0;
        HIPCHK(hipMemcpy(&slot, (const char *)(e->db.state + stream) + offsetof(StreamState, last_pm_slot), sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pm, e->db.pm + ((size_t)stream * NPM + slot) * PM_FRAME, PM_FRAME, hipMemcpyDeviceToHost));
    }
    if (bins) HIPCHK(hipMemcpy(bins, e->db.bins + (size_t)stream * NSYM * LIVE_N, (size_t)NSYM * LIVE_N * sizeof(float2), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_debug_fetch_costas(nrsc5hip_engine *e, int stream, float *freq, float *phase)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (!freq || !phase) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (e->staged_stream >= 0 && (rc = flush_staged(e))) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(freq, (const char *)(e->db.state + stream) + offsetof(StreamState, costas_freq), LIVE_N * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(phase, (const char *)(e->db.state + stream) + offsetof(StreamState, costas_phase), LIVE_N * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_debug_fetch_px(nrsc5hip_engine *e, int stream, int8_t *pair)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (!pair) FAIL(NRSC5HIP_EINVAL, "null argument");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pair, e->db.px_pair + (size_t)stream * 4 * PX_MAX, 4 * PX_MAX, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_debug_fetch_q15(nrsc5hip_engine *e, int stream, long long n, int16_t *out)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (n < 0 || n > e->db.q15_cap || !out) FAIL(NRSC5HIP_EINVAL, "bad argument");
    if (e->hc_stream == stream && (rc = hc_detach(e))) return rc;      // a stream that reads the pinned capture has no FIFO to show: it gets one (from its read position on)
    if (e->staged_stream >= 0 && (rc = flush_staged(e))) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, e->db.q15 + (size_t)stream * e->db.q15_cap, (size_t)n * sizeof(c16), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" void *nrsc5hip_debug_alloc_copy(const void *host, size_t nbytes)
{
    void *d = nullptr;
    if (hipMalloc(&d, nbytes ? nbytes : 1) != hipSuccess) return nullptr;
    if (host && hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    return d;
}

extern "C" void nrsc5hip_debug_free(void *dev) { (void)hipFree(dev); }

// Test / bench hygiene: overwrite every result buffer a pass writes (decoded-frame rings on the device, their pinned host mirror,
// the record rings) with a pattern no decode produces, so that a check after the next pass can only pass on bits written by it.
extern "C" int nrsc5hip_debug_poison_results(nrsc5hip_engine *e)
{
    ON_ENGINE_DEVICE(e);
    HIPCHK(hipDeviceSynchronize());
    const size_t S = e->cfg.max_streams;
    HIPCHK(hipMemset(e->db.p1_ring, 0xA5, S * e->db.p1_slots * (size_t)P1_WORDS * sizeof(uint32_t)));
    HIPCHK(hipMemset(e->db.records, 0, S * e->db.rec_cap * sizeof(BlockRecord)));
    HIPCHK(hipMemset(e->db.px_ring, 0xA5, S * (size_t)e->db.px_slots * 2 * PX_WORDS * sizeof(uint32_t)));
    if (e->frames_host) memset(e->frames_host, 0xA5, S * e->db.p1_slots * (size_t)P1_WORDS * sizeof(uint32_t));
    if (e->rec_host) memset(e->rec_host, 0, S * e->db.rec_cap * sizeof(BlockRecord));
    return 0;
}

extern "C" int nrsc5hip_stage_selftest(nrsc5hip_engine *e, int *failures)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !failures) FAIL(NRSC5HIP_EINVAL, "null argument");
    HIPCHK(hipMemsetAsync(e->db.counters + 2, 0, sizeof(int), e->main));
    launch_selftest(e->db.counters + 2, e->main);
    HIPCHK(hipMemcpyAsync(failures, e->db.counters + 2, sizeof(int), hipMemcpyDeviceToHost, e->main));
    HIPCHK(hipStreamSynchronize(e->main));
    return 0;
}

extern "C" int nrsc5hip_stage_math(nrsc5hip_engine *e, int fn, const void *a, const void *b, long long n, void *out0, void *out1)
{
    ON_ENGINE_DEVICE(e);
    if (fn < NRSC5HIP_MATH_REF_SINCOSF || fn > NRSC5HIP_MATH_SMALL_ATAN) FAIL(NRSC5HIP_EINVAL, "unknown function %d", fn);
    const bool two_in = fn == NRSC5HIP_MATH_REF_ATAN2F || fn == NRSC5HIP_MATH_FAST_ATAN2, two_out = !two_in && fn != NRSC5HIP_MATH_SMALL_ATAN;
    if (!a || !out0 || (two_in && !b) || (two_out && !out1) || n < 1 || n > (1LL << 28)) FAIL(NRSC5HIP_EINVAL, "bad argument");
    const size_t bytes = (size_t)n * (fn >= NRSC5HIP_MATH_SMALL_COS_SIN ? sizeof(double) : sizeof(float));
    DevTmp da, db, d0, d1;
    HIPCHK(hipMalloc(&da.p, bytes));
    HIPCHK(hipMalloc(&d0.p, bytes));
    HIPCHK(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice));
    if (two_in) { HIPCHK(hipMalloc(&db.p, bytes)); HIPCHK(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice)); }
    if (two_out) HIPCHK(hipMalloc(&d1.p, bytes));
    if (launch_stage_math(fn, da.p, db.p, n, d0.p, d1.p, e->main)) FAIL(NRSC5HIP_EINVAL, "unknown function %d", fn);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(out0, d0.p, bytes, hipMemcpyDeviceToHost));
    if (two_out) HIPCHK(hipMemcpy(out1, d1.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_stage_halfband_raw(nrsc5hip_engine *e, int form, const uint8_t *iq, size_t nbytes, int lead, long long a0, long long n, int16_t *out, uint32_t *probe)
{
    ON_ENGINE_DEVICE(e);
    if (form != NRSC5HIP_HB_ACQ && form != NRSC5HIP_HB_SYM128 && form != NRSC5HIP_HB_SYM256) FAIL(NRSC5HIP_EINVAL, "unknown form %d", form);
    if (!iq || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (lead != 0 && lead != 4 && lead != 8 && lead != 12) FAIL(NRSC5HIP_EINVAL, "lead %d: 0, 4, 8 or 12 bytes", lead);
    if (n < 1 || a0 < 0) FAIL(NRSC5HIP_EINVAL, "bad range");
    if (nbytes % 4 || nbytes > ((size_t)1 << 30)) FAIL(NRSC5HIP_EINVAL, "bad length");
    // decimated sample a reads the dwords a - 7 .. a of the capture (in front of the stream: history, never memory); a symbol workgroup reads nothing
    // beyond its own last sample's (raw_symbol_load / _load8), so the last output's dword bounds every read
    const long long dwords = (long long)(nbytes / 4), per = form == NRSC5HIP_HB_ACQ ? 1 : SYM_N;
    if (a0 > dwords || n > (dwords - a0) / per) FAIL(NRSC5HIP_EINVAL, "samples %lld + %lld x %lld reach beyond the %lld raw dwords", a0, n, per, dwords);
    const size_t nout = (size_t)(n * per), lanes = form == NRSC5HIP_HB_SYM256 ? 256 : 128;
    const bool probing = probe && form != NRSC5HIP_HB_ACQ;
    static const float probe_operands[4] = { 1.0f, 0x1.8p-24f, 0x1p-126f, 0.5f };   // 1 + 1.5 * 2^-24; 2^-126 * 0.5
    DevTmp draw, dout, dpc, dprobe;
    HIPCHK(hipMalloc(&draw.p, nbytes + 16));
    HIPCHK(hipMalloc(&dout.p, nout * sizeof(c16)));
    HIPCHK(hipMemcpy((uint8_t *)draw.p + lead, iq, nbytes, hipMemcpyHostToDevice));
    if (probing) {
        HIPCHK(hipMalloc(&dpc.p, sizeof(probe_operands)));
        HIPCHK(hipMalloc(&dprobe.p, (size_t)n * lanes * 4 * sizeof(uint32_t)));
        HIPCHK(hipMemcpy(dpc.p, probe_operands, sizeof(probe_operands), hipMemcpyHostToDevice));
    }
    if (form == NRSC5HIP_HB_ACQ) launch_stage_halfband_acq(e->tb, (const uint8_t *)draw.p + lead, a0, n, (c16 *)dout.p, e->main);
    else launch_stage_halfband_sym(e->tb, (int)lanes, (const uint8_t *)draw.p + lead, a0, (int)n, (c16 *)dout.p, (const float *)dpc.p, (uint32_t *)dprobe.p, e->main);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(out, dout.p, nout * sizeof(c16), hipMemcpyDeviceToHost));
    if (probing) HIPCHK(hipMemcpy(probe, dprobe.p, (size_t)n * lanes * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

// ---- the FEC stage on caller data (include/nrsc5hip.h; tests/fec_checks.py) ----------------------------------------------------------
// The production kernels run on stream 0 of the engine: the hook resets it, writes the hand-off words the block step would have left
// in its state, launches what launch_inorder_p1 / issue_step launch, and resets it again.  Nothing of the arithmetic lives here.
#define POKE(base, type, field, value) do { const decltype(type::field) _v = (value); HIPCHK(hipMemcpy((char *)(base) + offsetof(type, field), &_v, sizeof(_v), hipMemcpyHostToDevice)); } while (0)
#define POKE_AT(base, type, field, k, value) do { const int _v = (value); HIPCHK(hipMemcpy((char *)(base) + offsetof(type, field) + (k) * sizeof(int), &_v, sizeof(_v), hipMemcpyHostToDevice)); } while (0)

// stream 0, freshly reset, FM; the buffer table without the consumers a stage run must not feed (the L2 index, the host's frame mirror)
static int stage_stream0(nrsc5hip_engine *e, DevBuffers &db)
{
    int rc = check_stream(e, 0); if (rc) return rc;
    if (e->mode_host[0] != MODE_FM) FAIL(NRSC5HIP_EINVAL, "stream 0 must be in FM mode");
    if ((rc = nrsc5hip_stream_fresh(e, 0))) return rc;
    db = e->db;
    db.l2_ring = nullptr; db.l2_px_ring = nullptr; db.l2_am_ring = nullptr; db.p1_mirror = nullptr;
    return 0;
}

extern "C" int nrsc5hip_stage_p1_deint(nrsc5hip_engine *e, const int8_t *pm, uint32_t *out)
{
    ON_ENGINE_DEVICE(e);
    if (!pm || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    DevBuffers db; int rc = stage_stream0(e, db); if (rc) return rc;
    HIPCHK(hipMemcpy(db.pm, pm, PM_FRAME, hipMemcpyHostToDevice));            // matrix slot 0 of stream 0
    HIPCHK(hipMemset(db.coded, 0xA5, (size_t)P1_LEN * sizeof(int)));          // every dword must be written
    POKE_AT(db.state, StreamState, p1_pending, 0, 1);
    POKE_AT(db.state, StreamState, p1_pmslot, 0, 0);
    launch_p1_deint(e->tb, db, 1, nullptr, 0, 0, e->main);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(out, db.coded, (size_t)P1_LEN * sizeof(int), hipMemcpyDeviceToHost));
    return nrsc5hip_stream_fresh(e, 0);
}

extern "C" int nrsc5hip_stage_p1_frame(nrsc5hip_engine *e, const int8_t *soft, int walk, uint8_t *bits, int *errors)
{
    ON_ENGINE_DEVICE(e);
    if (!soft || !bits || !errors) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (walk != 0 && walk != 1) FAIL(NRSC5HIP_EINVAL, "walk %d: 0 (block-parallel traceback) or 1 (single-path walk)", walk);
    DevBuffers db; int rc = stage_stream0(e, db); if (rc) return rc;
    std::vector<int> words((size_t)P1_LEN);                                    // the dword per step k_p1_deint leaves for the forward pass
    for (int i = 0; i < P1_LEN; i++) words[i] = (int)((uint32_t)(uint8_t)soft[3 * i] | (uint32_t)(uint8_t)soft[3 * i + 1] << 8 | (uint32_t)(uint8_t)soft[3 * i + 2] << 16);
    HIPCHK(hipMemcpy(db.coded, words.data(), words.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(db.p1_ring, 0xA5, (size_t)P1_WORDS * sizeof(uint32_t)));
    const float poison = -1.0f;
    HIPCHK(hipMemcpy((char *)db.records + offsetof(BlockRecord, ber), &poison, sizeof(float), hipMemcpyHostToDevice));
    POKE_AT(db.state, StreamState, p1_pending, 0, 1);
    POKE_AT(db.state, StreamState, p1_slot, 0, 0);
    POKE_AT(db.state, StreamState, p1_record, 0, 0);
    const int segments = e->fwd_segments > 0 ? e->fwd_segments : 16;
    launch_p1_forward(e->tb, db, 1, nullptr, 0, 0, e->main, segments, e->fwd_warm);
    launch_p1_traceback(e->tb, db, 1, nullptr, 0, 0, e->main, 0, segments, walk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    std::vector<uint32_t> w((size_t)P1_WORDS);
    float ber = -1.0f;
    HIPCHK(hipMemcpy(w.data(), db.p1_ring, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&ber, (const char *)db.records + offsetof(BlockRecord, ber), sizeof(float), hipMemcpyDeviceToHost));
    if (ber < 0.0f) FAIL(NRSC5HIP_EHIP, "the traceback left no error count");
    nrsc5hip_unpack_bits(w.data(), P1_LEN, bits);
    // the record holds (float)count / 365440 (decode.c:458): count < 2^19, so the quotient's rounding error times 365440 is below 0.03 and the integer comes back exactly
    *errors = (int)llround((double)ber * P1_CODED);
    return nrsc5hip_stream_fresh(e, 0);
}

extern "C" int nrsc5hip_stage_pids(nrsc5hip_engine *e, const int8_t *pm, int bc, int8_t *coded, uint8_t *bits, int *crc_ok)
{
    ON_ENGINE_DEVICE(e);
    if (!pm || !coded || !bits || !crc_ok) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (bc < 0 || bc > 15) FAIL(NRSC5HIP_EINVAL, "block count %d out of range", bc);
    DevBuffers db; int rc = stage_stream0(e, db); if (rc) return rc;
    HIPCHK(hipMemcpy(db.pm, pm, PM_FRAME, hipMemcpyHostToDevice));
    const int rec0 = 0;
    const uint32_t clear[4] = { 0, 0, 0, 0 };
    HIPCHK(hipMemcpy((char *)db.records + offsetof(BlockRecord, flags), clear, sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((char *)db.records + offsetof(BlockRecord, pids), clear, 3 * sizeof(uint32_t), hipMemcpyHostToDevice));
    launch_stage_pids_gather(e->tb, db.pm, bc, db.pids_stage, e->main);         // window slot 0, frame slot 0 of stream 0
    HIPCHK(hipMemcpyAsync(db.pids_rec, &rec0, sizeof(int), hipMemcpyHostToDevice, e->main));
    launch_pids_decode(e->tb, db, 1, nullptr, 0, 1, e->main);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    BlockRecord rec;
    int left = 0;
    HIPCHK(hipMemcpy(coded, db.pids_stage, 3 * PIDS_LEN, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&rec, db.records, sizeof(rec), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&left, db.pids_rec, sizeof(int), hipMemcpyDeviceToHost));
    if (left != -1) FAIL(NRSC5HIP_EHIP, "the staged PIDS frame was not decoded");
    nrsc5hip_unpack_bits(rec.pids, PIDS_LEN, bits);
    *crc_ok = (rec.flags & REC_PIDS_CRC) ? 1 : 0;
    return nrsc5hip_stream_fresh(e, 0);
}

extern "C" int nrsc5hip_stage_px_interleave(nrsc5hip_engine *e, int len, int npairs, const int8_t *pairs, int8_t *out, int *ready)
{
    ON_ENGINE_DEVICE(e);
    if (!pairs || !out || !ready) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (len != PX_MAX && len != PX_MAX / 2) FAIL(NRSC5HIP_EINVAL, "frame length %d: %d or %d", len, PX_MAX / 2, PX_MAX);
    if (npairs < 1) FAIL(NRSC5HIP_EINVAL, "bad pair count");
    DevBuffers db; int rc = stage_stream0(e, db); if (rc) return rc;
    HIPCHK(hipMemset(db.px_mem, 0, (size_t)2 * PX_MEM));                      // a fresh interleaver: the reference's calloc'd memory
    POKE(db.state, StreamState, px_nch, 2);
    POKE(db.state, StreamState, px_record, 0);
    POKE(db.state, StreamState, px_slot, 0);
    for (int p = 0; p < npairs; p++) {
        for (int ch = 0; ch < 2; ch++)
            HIPCHK(hipMemcpy(db.px_pair + (size_t)ch * 2 * PX_MAX, pairs + ((size_t)p * 2 + ch) * 2 * len, (size_t)2 * len, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(db.px_stage, 0x5A, (size_t)2 * PX_DEPUNCT));
        POKE(db.state, StreamState, px_go, len);                               // k_px_commit clears it
        launch_px_deint(e->tb, db, 1, nullptr, 0, 0, e->main);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->main));
        PxJob job[2];
        HIPCHK(hipMemcpy(job, db.px_job, sizeof(job), hipMemcpyDeviceToHost));
        if ((job[0].rec < 0) != (job[1].rec < 0) || job[0].len != len || job[1].len != len) FAIL(NRSC5HIP_EHIP, "the two channels' jobs disagree");
        ready[p] = job[0].rec >= 0 ? 1 : 0;
        for (int ch = 0; ch < 2; ch++)
            HIPCHK(hipMemcpy(out + ((size_t)p * 2 + ch) * 3 * len, db.px_stage + (size_t)ch * PX_DEPUNCT, (size_t)3 * len, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemset(db.px_mem, 0, (size_t)2 * PX_MEM));
    HIPCHK(hipMemset(db.px_job, 0xff, 2 * sizeof(PxJob)));
    return nrsc5hip_stream_fresh(e, 0);
}

extern "C" int nrsc5hip_stage_am_deinterleave(nrsc5hip_engine *e, int psmi, int nframes, const uint8_t *sym, int8_t *v1, int8_t *v3)
{
    ON_ENGINE_DEVICE(e);
    if (!sym || !v1 || !v3) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (psmi != 1 && psmi != AM_MA3) FAIL(NRSC5HIP_EINVAL, "service mode %d: 1 (MA1) or 2 (MA3)", psmi);
    if (nframes < 1) FAIL(NRSC5HIP_EINVAL, "bad frame count");
    if (!e->db.am) FAIL(NRSC5HIP_EINVAL, "engine was created without am_enable");
    DevBuffers db; int rc = stage_stream0(e, db); if (rc) return rc;
    const size_t n3 = psmi == AM_MA3 ? (size_t)AM_VIT : (size_t)3 * AM_P3_LEN_MA1;
    HIPCHK(hipMemset(db.am_q, 0, (size_t)3 * 2 * AM_VIT));                    // a fresh delay ring: the reference's calloc'd delay lines
    POKE(db.state, StreamState, active, 1);
    POKE(db.am, AmStream, dec_bc, 7);
    POKE(db.am, AmStream, dec_psmi, psmi);
    POKE(db.am, AmStream, dec_rdbi, 0);
    POKE(db.am, AmStream, dec_record, 0);
    for (int f = 0; f < nframes; f++) {
        HIPCHK(hipMemcpy(db.am_sym, sym + (size_t)f * 4 * AM_SYMS, (size_t)4 * AM_SYMS, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(db.am_vit, 0x5A, (size_t)2 * AM_VIT));
        launch_am_interleave(e->tb, db, 1, nullptr, -1, 0, e->main);           // all AM_IL_PARTS slices; the last one commits (delay-line head)
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->main));
        HIPCHK(hipMemcpy(v1 + (size_t)f * AM_VIT, db.am_vit, AM_VIT, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(v3 + (size_t)f * n3, db.am_vit + AM_VIT, n3, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemset(db.am_q, 0, (size_t)3 * 2 * AM_VIT));
    HIPCHK(hipMemset(db.am_vit, 0, (size_t)2 * AM_VIT));
    return nrsc5hip_stream_fresh(e, 0);
}

extern "C" int nrsc5hip_stage_am_epilogue(nrsc5hip_engine *e, const int8_t *soft, const uint8_t *bits, int len, int code, int threads, int *errors,
                                          uint8_t *bits_out, uint32_t *words_out)
{
    ON_ENGINE_DEVICE(e);
    if (!soft || !bits || !errors || !bits_out || !words_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (threads != 64 && threads != 256) FAIL(NRSC5HIP_EINVAL, "workgroup size %d: 64 or 256", threads);
    // the frames of an AM L1 frame (am_decode_frame): P1 = role 0, E1; P3 = role 8: MA1 E2, MA3 E1
    int role, psmi;
    if (len == AM_P1_LEN && code == NRSC5HIP_CODE_E1) { role = 0; psmi = 1; }
    else if (len == AM_P3_LEN_MA1 && code == NRSC5HIP_CODE_E2) { role = 8; psmi = 1; }
    else if (len == AM_P3_LEN_MA3 && code == NRSC5HIP_CODE_E1) { role = 8; psmi = AM_MA3; }
    else FAIL(NRSC5HIP_EINVAL, "no AM frame of %d bits with code %d", len, code);
    const int words = (len + 31) / 32, word0 = role == 8 ? AM_P3_WORD0 : 0;
    static_assert(AM_P3_WORD0 + (AM_P3_LEN_MA3 + 31) / 32 <= P1_WORDS, "an AM L1 frame fits a frame slot");
    std::vector<uint32_t> w((size_t)P1_WORDS, 0xA5A5A5A5u);
    for (int k = 0; k < words; k++) w[word0 + k] = 0;
    for (int i = 0; i < len; i++) if (bits[i] & 1) w[word0 + (i >> 5)] |= 1u << (i & 31);
    if (len & 31) w[word0 + words - 1] |= ~((1u << (len & 31)) - 1u);            // the last word's bits beyond the frame arrive set: the descramble must clear them
    DevTmp dvit, dslot, derr;
    HIPCHK(hipMalloc(&dvit.p, (size_t)2 * AM_VIT));
    HIPCHK(hipMalloc(&dslot.p, (size_t)P1_WORDS * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&derr.p, sizeof(int)));
    HIPCHK(hipMemset(dvit.p, 0, (size_t)2 * AM_VIT));
    HIPCHK(hipMemset(derr.p, 0xff, sizeof(int)));
    HIPCHK(hipMemcpy((int8_t *)dvit.p + (role == 8 ? AM_VIT : 0), soft, (size_t)3 * len, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dslot.p, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    launch_stage_am_epilogue(e->tb, (const int8_t *)dvit.p, (uint32_t *)dslot.p, role, psmi, threads, (int *)derr.p, e->main);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(w.data(), dslot.p, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(errors, derr.p, sizeof(int), hipMemcpyDeviceToHost));
    for (int k = 0; k < P1_WORDS; k++) if ((k < word0 || k >= word0 + words) && w[k] != 0xA5A5A5A5u) FAIL(NRSC5HIP_EHIP, "the epilogue wrote word %d, outside its frame", k);
    memcpy(words_out, w.data() + word0, (size_t)words * sizeof(uint32_t));
    nrsc5hip_unpack_bits(w.data() + word0, len, bits_out);
    return 0;
}

// ---- coarse acquisition on caller data (include/nrsc5hip.h; tests/acq_checks.py) --------------------------------------------------------------
// launch_acquire / launch_am_step unchanged on freshly reset streams whose FIFO window (or attached capture), FIR history and sync state the hook
// wrote; everything the kernels leave is filled with ACQ_FILL bytes first, so a buffer a stream must not touch shows it.  Nothing of the arithmetic lives here.
constexpr int ACQ_FILL = 0xA5;

static int acq_check_common(nrsc5hip_engine *e, int n, const int *state, int mode, long long window)
{
    if (n < 1 || n > e->cfg.max_streams) FAIL(NRSC5HIP_EINVAL, "%d streams: 1 .. max_streams (%d)", n, e->cfg.max_streams);
    if (e->db.q15_cap < window) FAIL(NRSC5HIP_EINVAL, "q15_capacity %lld is smaller than a window (%lld)", e->db.q15_cap, window);
    for (int s = 0; s < n; s++) {
        if (state[s] != SYNC_NONE && state[s] != SYNC_COARSE && state[s] != SYNC_FINE) FAIL(NRSC5HIP_EINVAL, "stream %d: sync state %d: 0 (NONE), 1 (COARSE) or 2 (FINE)", s, state[s]);
        if (e->mode_host[s] != mode) FAIL(NRSC5HIP_EINVAL, "stream %d must be in %s mode", s, mode == MODE_AM ? "AM" : "FM");
    }
    return 0;
}

// history, sync state and the fill pattern over the three coarse_* words of stream s
static int acq_poke(nrsc5hip_engine *e, int s, const int16_t *hist, int state)
{
    char *st = (char *)(e->db.state + s);
    static_assert(offsetof(StreamState, coarse_im) - offsetof(StreamState, coarse_samperr) == 8, "coarse_samperr, coarse_re, coarse_im are three adjacent words");
    HIPCHK(hipMemcpy(st + offsetof(StreamState, fir_hist), hist, 31 * sizeof(c16), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(st + offsetof(StreamState, sync_state), &state, sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(st + offsetof(StreamState, coarse_samperr), ACQ_FILL, 12));
    return 0;
}

static int acq_peek(nrsc5hip_engine *e, int s, int *samperr, float *peak, int16_t *hist_out)
{
    const char *st = (const char *)(e->db.state + s);
    HIPCHK(hipMemcpy(samperr, st + offsetof(StreamState, coarse_samperr), sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(peak, st + offsetof(StreamState, coarse_re), 2 * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hist_out, st + offsetof(StreamState, fir_hist), 31 * sizeof(c16), hipMemcpyDeviceToHost));
    return 0;
}

// the FM launch and what it left, for streams 0 .. n-1 (acq_win: the zero-copy seam's decimated windows, or null)
static int acq_run_fm(nrsc5hip_engine *e, int n, int16_t *acq_win, int16_t *filt, float *sums, int *samperr, float *peak, int16_t *hist_out)
{
    HIPCHK(hipMemset(e->db.acq_filt, ACQ_FILL, (size_t)n * WIN_N * sizeof(c16)));
    HIPCHK(hipMemset(e->db.acq_sums, ACQ_FILL, (size_t)n * SYM_N * sizeof(float2)));
    if (acq_win) HIPCHK(hipMemset(e->db.acq_win, ACQ_FILL, (size_t)n * WIN_N * sizeof(c16)));
    launch_acquire(e->tb, e->db, n, nullptr, e->main);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(filt, e->db.acq_filt, (size_t)n * WIN_N * sizeof(c16), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sums, e->db.acq_sums, (size_t)n * SYM_N * sizeof(float2), hipMemcpyDeviceToHost));
    if (acq_win) HIPCHK(hipMemcpy(acq_win, e->db.acq_win, (size_t)n * WIN_N * sizeof(c16), hipMemcpyDeviceToHost));
    for (int s = 0; s < n; s++) { int rc = acq_peek(e, s, samperr + s, peak + 2 * s, hist_out + (size_t)s * 62); if (rc) return rc; }
    for (int s = 0; s < n; s++) { int rc = nrsc5hip_stream_fresh(e, s); if (rc) return rc; }
    return 0;
}

extern "C" int nrsc5hip_stage_acquire(nrsc5hip_engine *e, int n, const int16_t *win, const int16_t *hist, const int *state, const int *fill,
                                      int16_t *filt, float *sums, int *samperr, float *peak, int16_t *hist_out)
{
    ON_ENGINE_DEVICE(e);
    if (!win || !hist || !state || !fill || !filt || !sums || !samperr || !peak || !hist_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    int rc = acq_check_common(e, n, state, MODE_FM, WIN_N); if (rc) return rc;
    for (int s = 0; s < n; s++) if (fill[s] < 0 || fill[s] > WIN_N) FAIL(NRSC5HIP_EINVAL, "stream %d: fill %d: 0 .. %d samples", s, fill[s], WIN_N);
    for (int s = 0; s < n; s++) if ((rc = nrsc5hip_stream_fresh(e, s))) return rc;
    for (int s = 0; s < n; s++) {
        HIPCHK(hipMemcpy(e->db.q15 + (size_t)s * e->db.q15_cap, win + (size_t)s * WIN_N * 2, (size_t)WIN_N * sizeof(c16), hipMemcpyHostToDevice));
        POKE(e->db.state + s, StreamState, wr, (long long)fill[s]);
        if ((rc = acq_poke(e, s, hist + (size_t)s * 62, state[s]))) return rc;
    }
    return acq_run_fm(e, n, nullptr, filt, sums, samperr, peak, hist_out);
}

extern "C" int nrsc5hip_stage_acquire_raw(nrsc5hip_engine *e, int n, const uint8_t *iq, long long nbytes, const long long *rd, const int16_t *hist, const int *state,
                                          int16_t *acq_win, int16_t *filt, float *sums, int *samperr, float *peak, int16_t *hist_out)
{
    ON_ENGINE_DEVICE(e);
    if (!iq || !rd || !hist || !state || !acq_win || !filt || !sums || !samperr || !peak || !hist_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (!e->cfg.batch_zero_copy || !e->db.acq_win) FAIL(NRSC5HIP_EINVAL, "engine was created without batch_zero_copy");
    int rc = acq_check_common(e, n, state, MODE_FM, WIN_N); if (rc) return rc;
    if (nbytes < 4 || nbytes % 4 || nbytes > (1LL << 30)) FAIL(NRSC5HIP_EINVAL, "bad capture length %lld", nbytes);
    // decimated sample a reads the dwords a - 7 .. a of the capture (in front of it: history, never memory): the window's last sample bounds every read
    for (int s = 0; s < n; s++) if (rd[s] < 0 || 4 * (rd[s] + WIN_N) > nbytes) FAIL(NRSC5HIP_EINVAL, "stream %d: the window at %lld reaches beyond the %lld raw dwords", s, rd[s], nbytes / 4);
    DevTmp draw;
    HIPCHK(hipMalloc(&draw.p, (size_t)n * (size_t)nbytes));
    HIPCHK(hipMemcpy(draw.p, iq, (size_t)n * (size_t)nbytes, hipMemcpyHostToDevice));
    for (int s = 0; s < n; s++) if ((rc = nrsc5hip_stream_fresh(e, s))) return rc;
    std::vector<unsigned> counts((size_t)n, (unsigned)nbytes);
    HIPCHK(hipMemcpy(e->nbytes_dev, counts.data(), counts.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    launch_attach_raw(e->db, n, nullptr, (const uint8_t *)draw.p, nbytes, e->nbytes_dev, e->main);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    for (int s = 0; s < n; s++) {
        POKE(e->db.state + s, StreamState, rd, rd[s]);
        if ((rc = acq_poke(e, s, hist + (size_t)s * 62, state[s]))) return rc;
    }
    return acq_run_fm(e, n, acq_win, filt, sums, samperr, peak, hist_out);      // (the reset detaches the captures before draw is freed)
}

extern "C" int nrsc5hip_stage_am_acquire(nrsc5hip_engine *e, const int16_t *win, const int16_t *hist, int state, int fill, int *samperr, float *peak, int16_t *hist_out)
{
    ON_ENGINE_DEVICE(e);
    if (!win || !hist || !samperr || !peak || !hist_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (!e->db.am) FAIL(NRSC5HIP_EINVAL, "engine was created without am_enable");
    int rc = acq_check_common(e, 1, &state, MODE_AM, AM_WIN); if (rc) return rc;
    if (fill < 0 || fill > AM_WIN) FAIL(NRSC5HIP_EINVAL, "fill %d: 0 .. %d samples", fill, AM_WIN);
    if ((rc = nrsc5hip_stream_fresh(e, 0))) return rc;
    DevBuffers db = e->db;                                                     // without the consumers a stage run must not feed (stage_stream0)
    db.l2_ring = nullptr; db.l2_px_ring = nullptr; db.l2_am_ring = nullptr; db.p1_mirror = nullptr;
    HIPCHK(hipMemcpy(db.q15, win, (size_t)AM_WIN * sizeof(c16), hipMemcpyHostToDevice));
    POKE(db.state, StreamState, wr, (long long)fill);
    if ((rc = acq_poke(e, 0, hist, state))) return rc;
    HIPCHK(hipMemsetAsync(db.counters, 0, 4 * sizeof(int), e->main));
    // the launch form follows the engine, as in run_steps_am: k_am_block<512> for the window pipeline (p1_async; window 0, slot 0), k_am_block<256> in order
    launch_am_step(e->tb, db, 1, nullptr, e->main, e->cfg.l2_feedback, e->cfg.p1_async ? 0 : -1, 0, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    if ((rc = acq_peek(e, 0, samperr, peak, hist_out))) return rc;
    return nrsc5hip_stream_fresh(e, 0);
}

// ---- the AM block step on caller data (include/nrsc5hip.h; tests/am_checks.py) ----------------------------------------------------------------------
// k_am_block alone (launch_stage_am_block: the launch shapes of launch_am_step) on stream 0, freshly reset, whose window, history and state words the hook wrote;
// the record, the symbol matrices, the staged PIDS bytes and the dump buffers are filled with ACQ_FILL bytes first.  Nothing of the arithmetic lives here.
static void am_block_state_out(const StreamState &st, const AmStream &am, nrsc5hip_am_block_state *o)
{
    o->sync_state = st.sync_state; o->samperr = st.samperr; o->cfo = st.cfo; o->psmi = st.psmi; o->bc = st.bc; o->cfo_wait = st.cfo_wait;
    o->prev_angle = st.prev_angle; o->angle = st.angle; o->theta = st.theta;
    o->coarse_samperr = st.coarse_samperr; o->coarse_re = st.coarse_re; o->coarse_im = st.coarse_im; o->keep_extra = st.keep_extra;
    o->offset_history = am.offset_history; o->rdbi = am.rdbi; o->pli = am.pli; o->hppi = am.hppi; o->aabi = am.aabi;
    o->am_diversity_wait = am.am_diversity_wait; o->am_errors = am.am_errors;
    o->fine_epoch = st.fine_epoch; o->active = st.active; o->nblocks = st.nblocks; o->rd = st.rd;
}

extern "C" int nrsc5hip_stage_am_block(nrsc5hip_engine *e, const int16_t *win, const int16_t *hist, const nrsc5hip_am_block_state *in, int fill, int dump,
                                       nrsc5hip_record *rec, nrsc5hip_am_block_state *out, uint8_t *am_sym, int8_t *pids_stage, float *spectra, float *mult)
{
    ON_ENGINE_DEVICE(e);
    static_assert(sizeof(nrsc5hip_record) == sizeof(BlockRecord), "the public record mirrors BlockRecord");
    if (!win || !hist || !in || !rec || !out || !am_sym || !pids_stage || (dump && (!spectra || !mult))) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (!e->db.am) FAIL(NRSC5HIP_EINVAL, "engine was created without am_enable");
    int rc = acq_check_common(e, 1, &in->sync_state, MODE_AM, AM_WIN); if (rc) return rc;
    if (fill < 0 || fill > AM_WIN) FAIL(NRSC5HIP_EINVAL, "fill %d: 0 .. %d samples", fill, AM_WIN);
    if (in->bc < 0 || in->bc > 7) FAIL(NRSC5HIP_EINVAL, "block count %d: 0 .. 7", in->bc);
    // the fold reads win[31 * AM_SYM + AM_SYM - 1 + samperr] at most: samperr = AM_SYM / 2 + st.samperr (FINE) or coarse_samperr must stay in 0 .. AM_SYM
    if (in->samperr < -AM_SYM / 2 || in->samperr > AM_SYM / 2) FAIL(NRSC5HIP_EINVAL, "samperr %d: %d .. %d", in->samperr, -AM_SYM / 2, AM_SYM / 2);
    if (in->coarse_samperr < 0 || in->coarse_samperr >= AM_SYM) FAIL(NRSC5HIP_EINVAL, "coarse_samperr %d: 0 .. %d", in->coarse_samperr, AM_SYM - 1);
    if ((rc = nrsc5hip_stream_fresh(e, 0))) return rc;
    DevBuffers db = e->db;                                                     // without the consumers a stage run must not feed (stage_stream0), and without the replay
    db.l2_ring = nullptr; db.l2_px_ring = nullptr; db.l2_am_ring = nullptr; db.p1_mirror = nullptr; db.am_ckpt = nullptr;
    const int pipeline = e->cfg.p1_async ? 1 : 0;
    StreamState st; AmStream am;
    HIPCHK(hipMemcpy(&st, db.state, sizeof(st), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&am, db.am, sizeof(am), hipMemcpyDeviceToHost));
    st.wr = fill;
    memcpy(st.fir_hist, hist, sizeof(st.fir_hist));
    st.sync_state = in->sync_state; st.samperr = in->samperr; st.cfo = in->cfo; st.psmi = in->psmi; st.bc = in->bc; st.cfo_wait = in->cfo_wait;
    st.prev_angle = in->prev_angle; st.angle = in->angle; st.theta = in->theta;
    st.coarse_samperr = in->coarse_samperr; st.coarse_re = in->coarse_re; st.coarse_im = in->coarse_im; st.keep_extra = in->keep_extra;
    am.offset_history = in->offset_history; am.rdbi = in->rdbi; am.pli = in->pli; am.hppi = in->hppi; am.aabi = in->aabi;
    am.am_diversity_wait = in->am_diversity_wait; am.am_errors = in->am_errors;
    HIPCHK(hipMemcpy(db.state, &st, sizeof(st), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db.am, &am, sizeof(am), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db.q15, win, (size_t)AM_WIN * sizeof(c16), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(db.records, ACQ_FILL, sizeof(BlockRecord)));
    HIPCHK(hipMemset(db.am_sym, ACQ_FILL, (size_t)4 * AM_SYMS));
    HIPCHK(hipMemset(db.am_pids_stage, ACQ_FILL, (size_t)3 * PIDS_LEN));           // window parity 0, slot 0 of stream 0
    DevTmp dx, dm;
    if (dump) {
        HIPCHK(hipMalloc(&dx.p, (size_t)NSYM * AM_FFT * sizeof(float2)));
        HIPCHK(hipMalloc(&dm.p, (size_t)4 * AM_PW * sizeof(float2)));
        HIPCHK(hipMemset(dx.p, ACQ_FILL, (size_t)NSYM * AM_FFT * sizeof(float2)));
        HIPCHK(hipMemset(dm.p, ACQ_FILL, (size_t)4 * AM_PW * sizeof(float2)));
    }
    HIPCHK(hipMemsetAsync(db.counters, 0, 4 * sizeof(int), e->main));
    launch_stage_am_block(e->tb, db, pipeline, (float2 *)dx.p, (float2 *)dm.p, e->main);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(&st, db.state, sizeof(st), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&am, db.am, sizeof(am), hipMemcpyDeviceToHost));
    am_block_state_out(st, am, out);
    HIPCHK(hipMemcpy(rec, db.records, sizeof(BlockRecord), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(am_sym, db.am_sym, (size_t)4 * AM_SYMS, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pids_stage, db.am_pids_stage, (size_t)3 * PIDS_LEN, hipMemcpyDeviceToHost));
    if (dump) {
        HIPCHK(hipMemcpy(spectra, dx.p, (size_t)NSYM * AM_FFT * sizeof(float2), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(mult, dm.p, (size_t)4 * AM_PW * sizeof(float2), hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemset(db.am_sym, 0, (size_t)4 * AM_SYMS));                       // as the engine's creation leaves them
    HIPCHK(hipMemset(db.am_pids_stage, 0, (size_t)3 * PIDS_LEN));
    HIPCHK(hipMemset(db.records, 0, sizeof(BlockRecord)));
    return nrsc5hip_stream_fresh(e, 0);
}

extern "C" int nrsc5hip_debug_fetch_am_sym(nrsc5hip_engine *e, int stream, uint8_t *sym)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (!sym) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (!e->db.am_sym) FAIL(NRSC5HIP_EINVAL, "engine was created without am_enable");
    if (e->staged_stream >= 0 && (rc = flush_staged(e))) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(sym, e->db.am_sym + (size_t)stream * 4 * AM_SYMS, (size_t)4 * AM_SYMS, hipMemcpyDeviceToHost));
    return 0;
}

// ---- the exact oscillator on caller data (include/nrsc5hip.h; tests/nco_checks.py) --------------------------------------------------------------
// launch_nco_exact unchanged on streams 0 .. n-1, freshly reset, into whose state the hook wrote what prepare_block leaves for the kernel; the streams' table rows are
// filled with ACQ_FILL bytes first.  Nothing of the arithmetic lives here.
extern "C" int nrsc5hip_stage_nco_exact(nrsc5hip_engine *e, int n, const float *start, const float *inc, const int *active, const int *nco_mode, float *tab, float *end)
{
    ON_ENGINE_DEVICE(e);
    if (!start || !inc || !active || !nco_mode || !tab || !end) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (n < 1 || n > e->cfg.max_streams) FAIL(NRSC5HIP_EINVAL, "%d streams: 1 .. max_streams (%d)", n, e->cfg.max_streams);
    if (!e->db.nco_tab) FAIL(NRSC5HIP_EINVAL, "the engine has no oscillator table");
    int rc;
    for (int s = 0; s < n; s++) {
        if (e->mode_host[s] != MODE_FM) FAIL(NRSC5HIP_EINVAL, "stream %d must be in FM mode", s);
        if ((rc = nrsc5hip_stream_fresh(e, s))) return rc;
    }
    const size_t row = (size_t)NSYM * SYM_N;
    HIPCHK(hipMemset(e->db.nco_tab, ACQ_FILL, (size_t)n * row * sizeof(float2)));
    for (int s = 0; s < n; s++) {
        POKE(e->db.state + s, StreamState, active, active[s] ? 1 : 0);
        POKE(e->db.state + s, StreamState, nco_mode, nco_mode[s] ? 1 : 0);
        POKE(e->db.state + s, StreamState, nco_re, start[2 * s]);
        POKE(e->db.state + s, StreamState, nco_im, start[2 * s + 1]);
        POKE(e->db.state + s, StreamState, inc_re, inc[2 * s]);
        POKE(e->db.state + s, StreamState, inc_im, inc[2 * s + 1]);
    }
    launch_nco_exact(e->db, n, nullptr, e->main);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(tab, e->db.nco_tab, (size_t)n * row * sizeof(float2), hipMemcpyDeviceToHost));
    static_assert(offsetof(StreamState, nco_im) - offsetof(StreamState, nco_re) == 4, "nco_re, nco_im are adjacent words");
    for (int s = 0; s < n; s++) HIPCHK(hipMemcpy(end + 2 * s, (const char *)(e->db.state + s) + offsetof(StreamState, nco_re), 2 * sizeof(float), hipMemcpyDeviceToHost));
    for (int s = 0; s < n; s++) if ((rc = nrsc5hip_stream_fresh(e, s))) return rc;
    return 0;
}

// ---- the FM symbol transform on caller data (include/nrsc5hip.h; tests/sym_checks.py) -----------------------------------------------------------------
// launch_mixfft unchanged on streams 0 .. n-1, freshly reset, whose samples (an attached cu8 capture or a FIFO window) and block parameters the hook wrote; the bins of
// every stream of the engine are filled with ACQ_FILL bytes first.  Nothing of the arithmetic lives here.
static void sym_params_out(const StreamState &st, nrsc5hip_sym_params *o)
{
    o->a00 = (st.rd - st.base) + st.samperr_cur; o->dtheta = st.dtheta; o->theta = st.theta; o->growth = st.growth; o->active = st.active; o->nco_mode = st.nco_mode;
}

extern "C" int nrsc5hip_stage_symbols(nrsc5hip_engine *e, int n, int form, int params_mode, int prepare, const nrsc5hip_sym_stream *in, const int *ids,
                                      float *bins, nrsc5hip_sym_params *out)
{
    ON_ENGINE_DEVICE(e);
    if (!in || !bins || !out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (n < 1 || n > e->cfg.max_streams) FAIL(NRSC5HIP_EINVAL, "%d streams: 1 .. max_streams (%d)", n, e->cfg.max_streams);
    if (form != 1 && form != 2 && form != 4 && form != 8 && form != 16 && form != 32) FAIL(NRSC5HIP_EINVAL, "form %d: 1, 2, 4, 8, 16 or 32", form);
    if ((params_mode != 0 && params_mode != 1) || (prepare != 0 && prepare != 1)) FAIL(NRSC5HIP_EINVAL, "params_mode %d, prepare %d: 0 or 1", params_mode, prepare);
    if (ids) {
        std::vector<int> seen((size_t)n, 0);
        for (int k = 0; k < n; k++) { if (ids[k] < 0 || ids[k] >= n || seen[ids[k]]++) FAIL(NRSC5HIP_EINVAL, "ids must be a permutation of 0 .. %d", n - 1); }
    }
    const long long block = (long long)NSYM * SYM_N;
    size_t raw_total = 0;
    std::vector<size_t> raw_off((size_t)n, 0);
    for (int s = 0; s < n; s++) {
        const nrsc5hip_sym_stream &c = in[s];
        if (e->mode_host[s] != MODE_FM) FAIL(NRSC5HIP_EINVAL, "stream %d must be in FM mode", s);
        if ((c.raw != nullptr) == (c.q15 != nullptr)) FAIL(NRSC5HIP_EINVAL, "stream %d: a cu8 capture or a Q15 window, one of the two", s);
        long long have;
        if (c.raw) {
            if (c.lead != 0 && c.lead != 4 && c.lead != 8 && c.lead != 12) FAIL(NRSC5HIP_EINVAL, "stream %d: lead %d: 0, 4, 8 or 12 bytes", s, c.lead);
            if (c.raw_bytes % 4 || c.raw_bytes > ((size_t)1 << 30)) FAIL(NRSC5HIP_EINVAL, "stream %d: bad capture length", s);
            have = (long long)(c.raw_bytes / 4);
            raw_off[s] = raw_total;
            raw_total += (c.raw_bytes + 16 + 15) & ~(size_t)15;
        } else {
            if (c.q15_samples < 0 || c.q15_samples > e->db.q15_cap) FAIL(NRSC5HIP_EINVAL, "stream %d: %lld samples: 0 .. q15_capacity (%lld)", s, c.q15_samples, e->db.q15_cap);
            have = c.q15_samples;
        }
        // decimated sample a reads the dwords a - 7 .. a of a capture (in front of it: history, never memory) and a workgroup nothing beyond its symbol's last sample
        // (raw_symbol_load / _load8; the FIFO path reads win[0 .. 2159]): the last symbol's last sample bounds every read
        long long a00;
        if (params_mode == 0) {
            a00 = c.a00;
            if (c.nco_mode && !c.nco_tab) FAIL(NRSC5HIP_EINVAL, "stream %d: exact-oscillator mode without a table", s);
        } else {
            if (c.rd < 0 || c.wr > have || c.wr - c.rd < WIN_N) FAIL(NRSC5HIP_EINVAL, "stream %d: rd %lld, wr %lld: a complete window inside the %lld samples given", s, c.rd, c.wr, have);
            if (c.samperr < -SYM_N / 2 || c.samperr > SYM_N / 2) FAIL(NRSC5HIP_EINVAL, "stream %d: samperr %d: %d .. %d", s, c.samperr, -SYM_N / 2, SYM_N / 2);
            a00 = c.rd + SYM_N / 2 + c.samperr;                                   // acquire.c:112 (prepare_values)
        }
        if (a00 < 0 || a00 > have || block > have - a00) FAIL(NRSC5HIP_EINVAL, "stream %d: symbols at %lld reach beyond the %lld samples given", s, a00, have);
        if (c.nco_tab && !e->db.nco_tab) FAIL(NRSC5HIP_EINVAL, "the engine has no oscillator table");
    }
    int rc;
    for (int s = 0; s < n; s++) if ((rc = nrsc5hip_stream_fresh(e, s))) return rc;
    DevTmp draw;
    if (raw_total) HIPCHK(hipMalloc(&draw.p, raw_total));
    const size_t row = (size_t)NSYM * SYM_N, S = (size_t)e->cfg.max_streams;
    for (int s = 0; s < n; s++) {
        const nrsc5hip_sym_stream &c = in[s];
        StreamState st;
        HIPCHK(hipMemcpy(&st, e->db.state + s, sizeof(st), hipMemcpyDeviceToHost));
        if (c.raw) {
            uint8_t *at = (uint8_t *)draw.p + raw_off[s] + c.lead;
            HIPCHK(hipMemcpy(at, c.raw, c.raw_bytes, hipMemcpyHostToDevice));
            st.raw = at; st.wr = (long long)(c.raw_bytes / 4); st.base = 0;         // k_attach_raw
        } else {
            if (c.q15_samples) HIPCHK(hipMemcpy(e->db.q15 + (size_t)s * e->db.q15_cap, c.q15, (size_t)c.q15_samples * sizeof(c16), hipMemcpyHostToDevice));
            st.wr = c.q15_samples;
        }
        if (c.nco_tab) HIPCHK(hipMemcpy(e->db.nco_tab + (size_t)s * row, c.nco_tab, row * sizeof(float2), hipMemcpyHostToDevice));
        st.theta = c.theta;
        if (params_mode == 0) {
            st.rd = c.a00; st.samperr_cur = 0; st.dtheta = c.dtheta; st.growth = c.growth; st.active = c.active ? 1 : 0; st.nco_mode = c.nco_mode ? 1 : 0;
        } else {
            st.sync_state = SYNC_FINE; st.samperr = c.samperr; st.cfo = c.cfo; st.angle = c.angle; st.prev_angle = c.prev_angle; st.rd = c.rd; st.wr = c.wr;
            st.nco_exact = 0;                                                      // a FINE stream's blocks run on the closed form (what local_prepare assumes)
        }
        HIPCHK(hipMemcpy(e->db.state + s, &st, sizeof(st), hipMemcpyHostToDevice));
    }
    const int *ids_dev = nullptr;
    if (ids) { HIPCHK(hipMemcpy(e->ids_dev, ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice)); ids_dev = e->ids_dev; }
    const size_t bins_bytes = S * NSYM * LIVE_N * sizeof(float2);
    HIPCHK(hipMemset(e->db.bins, ACQ_FILL, bins_bytes));
    HIPCHK(hipMemsetAsync(e->db.counters, 0, 4 * sizeof(int), e->main));
    const int local = params_mode == 1 && prepare == 1;
    if (params_mode == 1 && !local) launch_prepare(e->db, n, ids_dev, 0, e->main);
    launch_mixfft(e->tb, e->db, n, ids_dev, e->main, form, local);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(bins, e->db.bins, bins_bytes, hipMemcpyDeviceToHost));
    if (local) {                                                                   // the commit the block step behind the kernel makes (prepare_block): the same values, now readable
        launch_prepare(e->db, n, ids_dev, 0, e->main);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->main));
    }
    for (int s = 0; s < n; s++) {
        StreamState st;
        HIPCHK(hipMemcpy(&st, e->db.state + s, sizeof(st), hipMemcpyDeviceToHost));
        sym_params_out(st, out + s);
    }
    if (params_mode == 1) for (int s = 0; s < n; s++) HIPCHK(hipMemset(e->db.records + (size_t)s * e->db.rec_cap, 0, sizeof(BlockRecord)));   // record slot 0: as the engine's creation leaves it
    HIPCHK(hipMemset(e->db.counters, 0, 4 * sizeof(int)));
    HIPCHK(hipMemset(e->db.bins, 0, bins_bytes));
    for (int s = 0; s < n; s++) if ((rc = nrsc5hip_stream_fresh(e, s))) return rc;  // (detaches the captures before draw is freed)
    return 0;
}

extern "C" int nrsc5hip_stage_viterbi_k7_debug(nrsc5hip_engine *e, const int8_t *soft, int len, uint8_t *bits, unsigned long long *dec_out)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !soft || !bits || !dec_out || len < 64) FAIL(NRSC5HIP_EINVAL, "bad argument");
    int8_t *dsoft = nullptr; unsigned long long *ddec = nullptr; uint32_t *dout = nullptr;
    const int words = (len + 31) / 32;
    HIPCHK(hipMalloc((void **)&dsoft, (size_t)3 * len));
    HIPCHK(hipMalloc((void **)&ddec, (size_t)(len + 64) * sizeof(unsigned long long)));
    HIPCHK(hipMalloc((void **)&dout, (size_t)words * sizeof(uint32_t)));
    HIPCHK(hipMemcpy(dsoft, soft, (size_t)3 * len, hipMemcpyHostToDevice));
    if (launch_viterbi_frames(e->vit_scratch, dsoft, len, 1, ddec, dout, e->main)) FAIL(NRSC5HIP_EINVAL, "frame length %d not supported or out of device memory", len);
    HIPCHK(hipStreamSynchronize(e->main));
    std::vector<uint32_t> w(words);
    HIPCHK(hipMemcpy(w.data(), dout, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dec_out, ddec, (size_t)(len + 64) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    nrsc5hip_unpack_bits(w.data(), len, bits);
    (void)hipFree(dsoft); (void)hipFree(ddec); (void)hipFree(dout);
    return 0;
}

// micro-benchmark: nframes random frames, `phases` bit0 = forward pass, bit1 = traceback; ms per launch
extern "C" int nrsc5hip_stage_viterbi_bench(nrsc5hip_engine *e, int len, int nframes, int phases, int reps, float *ms_per_launch)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !ms_per_launch || len < 64 || nframes < 1 || reps < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    int8_t *dsoft = nullptr; unsigned long long *ddec = nullptr; uint32_t *dout = nullptr;
    const int words = (len + 31) / 32;
    std::vector<int8_t> h((size_t)nframes * 3 * len);
    unsigned x = 12345;
    for (auto &v : h) { x = x * 1664525u + 1013904223u; v = (int8_t)((int)(x >> 24) - 128); if (v == -128) v = -127; }
    HIPCHK(hipMalloc((void **)&dsoft, h.size()));
    HIPCHK(hipMalloc((void **)&ddec, (size_t)nframes * (len + 64) * sizeof(unsigned long long)));
    HIPCHK(hipMalloc((void **)&dout, (size_t)nframes * words * sizeof(uint32_t)));
    HIPCHK(hipMemcpy(dsoft, h.data(), h.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ddec, 0x55, (size_t)nframes * (len + 64) * sizeof(unsigned long long)));
    hipEvent_t a, b; HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    const int seg = e->fwd_segments > 0 ? e->fwd_segments : 1;
    if (launch_viterbi_frames(e->vit_scratch, dsoft, len, nframes, ddec, dout, e->main, phases | 1 | (e->tb_walk ? 0 : 16), seg)) FAIL(NRSC5HIP_EINVAL, "frame length %d not supported or out of device memory", len);      // warm-up; packs the soft words and leaves decisions behind
    HIPCHK(hipEventRecord(a, e->main));
    for (int r = 0; r < reps; r++) {
        // a traceback-only measurement consumes the decisions in place: re-run the (untimed-irrelevant) forward pass is not possible
        // without timing it, so phases == 2 measures forward + traceback minus nothing -- callers subtract the forward figure
        (void)launch_viterbi_frames(e->vit_scratch, dsoft, len, nframes, ddec, dout, e->main, ((phases & 2) ? (phases | 1) : phases) | 8 | (e->tb_walk ? 0 : 16), seg);
    }
    HIPCHK(hipEventRecord(b, e->main));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, a, b));
    *ms_per_launch = ms / reps;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipFree(dsoft); (void)hipFree(ddec); (void)hipFree(dout);
    return 0;
}

// micro-benchmark of the K=9 trellis kernel (E2 code) on random hard-decision frames: phases bit0 = forward, bit1 = traceback
extern "C" int nrsc5hip_stage_viterbi_k9_bench(nrsc5hip_engine *e, int len, int nframes, int phases, int reps, float *ms_per_launch)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !ms_per_launch || len < 128 || nframes < 1 || reps < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    int8_t *dsoft = nullptr; unsigned long long *ddec = nullptr; uint32_t *dout = nullptr;
    const int words = (len + 31) / 32;
    // tail-biting code words of random payloads (generators 0561 / 0753 / 0711, bit 8 - k of the register = payload bit i - k),
    // one sign in 16 flipped: what the decoder sees on a healthy channel (pure noise would make every segment speculation fail)
    std::vector<int8_t> h((size_t)nframes * 3 * len);
    std::vector<uint8_t> pay((size_t)len);
    const unsigned gens[3] = { 0561, 0753, 0711 };
    unsigned x = 4321;
    for (int f = 0; f < nframes; f++) {
        for (auto &v : pay) { x = x * 1664525u + 1013904223u; v = (uint8_t)((x >> 24) & 1u); }
        for (int i = 0; i < len; i++) {
            unsigned r = 0;
            for (int k = 0; k < 9; k++) r |= (unsigned)pay[(size_t)((i - k + len) % len)] << (8 - k);
            for (int j = 0; j < 3; j++) {
                x = x * 1664525u + 1013904223u;
                int v = (__builtin_popcount(r & gens[j]) & 1) ? 1 : -1;
                if (((x >> 20) & 15u) == 0) v = -v;
                h[((size_t)f * len + i) * 3 + j] = (int8_t)v;
            }
        }
    }
    HIPCHK(hipMalloc((void **)&dsoft, h.size()));
    HIPCHK(hipMalloc((void **)&ddec, (size_t)nframes * 4 * (len + 64) * sizeof(unsigned long long)));
    HIPCHK(hipMalloc((void **)&dout, (size_t)nframes * words * sizeof(uint32_t)));
    HIPCHK(hipMemcpy(dsoft, h.data(), h.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ddec, 0x55, (size_t)nframes * 4 * (len + 64) * sizeof(unsigned long long)));
    K9Meta *dmeta = nullptr;
    if (e->am_segments > 1) HIPCHK(hipMalloc((void **)&dmeta, (size_t)nframes * sizeof(K9Meta)));
    hipEvent_t a, b; HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    launch_viterbi_k9_frames(dsoft, len, nframes, 0561, 0753, 0711, ddec, dout, e->main, 3, dmeta, e->am_segments, e->am_warm, e->am_runin, e->db.am_k9stats);
    HIPCHK(hipEventRecord(a, e->main));
    for (int r = 0; r < reps; r++) launch_viterbi_k9_frames(dsoft, len, nframes, 0561, 0753, 0711, ddec, dout, e->main, phases, dmeta, e->am_segments, e->am_warm, e->am_runin, e->db.am_k9stats);
    HIPCHK(hipEventRecord(b, e->main));
    HIPCHK(hipEventSynchronize(b));
    if (dmeta) (void)hipFree(dmeta);
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, a, b));
    *ms_per_launch = ms / reps;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipFree(dsoft); (void)hipFree(ddec); (void)hipFree(dout);
    return 0;
}

// Tuning knobs and test hooks: an explicit entry point, nothing is read from the environment.
extern "C" int nrsc5hip_debug_tune(nrsc5hip_engine *e, int knob, int value)
{
    ON_ENGINE_DEVICE(e);
    if (!e) FAIL(NRSC5HIP_EINVAL, "null engine");
    HIPCHK(hipDeviceSynchronize());
    switch (knob) {
    case NRSC5HIP_TUNE_DECODE_STREAMS:    e->naux = std::min(std::max(value, 1), NAUX); break;
    case NRSC5HIP_TUNE_AM_DECODE_STREAMS: e->naux_am = std::min(std::max(value, 1), NAUX); break;
    case NRSC5HIP_TUNE_VERDICT_LAG:       e->verdict_lag = std::min(std::max(value, 0), NWIN); break;
    case NRSC5HIP_TUNE_FWD_SEGMENTS:      e->fwd_segments = std::min(std::max(value, 0), VIT3_GMAX); break;
    case NRSC5HIP_TUNE_FWD_WARM:          e->fwd_warm = value > 0 ? 2 : 0; break;
    case NRSC5HIP_TUNE_DECODE_CUS: {
        // decode streams confined to value / 32 of the CUs (the pattern keeps that share of every XCD whichever way mask bits map to CUs)
        const int k = std::min(std::max(value, 8), 32) & ~7;
        hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, e->cfg.device));
        const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
        std::vector<uint32_t> mask((size_t)words, 0u);
        for (int i = 0; i < ncu; i++) if ((i % 32) < k) mask[(size_t)i / 32] |= 1u << (i % 32);
        for (int a = 0; a < NAUX; a++) {                       // the new stream first; the old one is destroyed only once it exists
            hipStream_t fresh = nullptr;
            if (k >= 32) HIPCHK(hipStreamCreate(&fresh));
            else HIPCHK(hipExtStreamCreateWithCUMask(&fresh, (uint32_t)words, mask.data()));
            (void)hipStreamDestroy(e->aux[a]);
            e->aux[a] = fresh;
        }
        break;
    }
    case NRSC5HIP_TUNE_DECODE_PRIORITY: {
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        for (int a = 0; a < NAUX; a++) {
            hipStream_t fresh = nullptr;
            if (value) HIPCHK(hipStreamCreateWithPriority(&fresh, hipStreamDefault, least));
            else HIPCHK(hipStreamCreate(&fresh));
            (void)hipStreamDestroy(e->aux[a]);
            e->aux[a] = fresh;
        }
        break;
    }
    case NRSC5HIP_TUNE_TRACEBACK_WALK:    e->tb_walk = std::min(std::max(value, 0), 16384); break;
    case NRSC5HIP_TUNE_SYNC_LANES:        e->sync_lanes = (value == 256 || value == 768) ? value : 0; break;
    case NRSC5HIP_TUNE_SEAM_PREPARE:      e->fuse_seam_prepare = value != 0; break;
    case NRSC5HIP_TUNE_FOLD_REPORT:       e->fold_report = value != 0; break;
    case NRSC5HIP_TUNE_NCO_EXACT:         e->db.nco_policy = e->db.nco_tab ? std::min(std::max(value, 0), (int)NCO_EXACT_ALWAYS) : (int)NCO_CLOSED_FORM; break;
    case NRSC5HIP_TUNE_FLOW_MIN:          e->flow_min = std::max(value, 0); break;
    case NRSC5HIP_TUNE_LOOP_EXACT:        e->db.loop_exact = std::min(std::max(value, 0), 2); break;
    case NRSC5HIP_TUNE_EARLY_FLUSH_KB:    e->early_flush = (size_t)std::max(value, 0) << 10; break;
    case NRSC5HIP_TUNE_DEFER_WAIT:        e->defer_wait = value != 0; break;
    case NRSC5HIP_TUNE_DIRECT_DECIMATE:   e->direct_decimate = value != 0; break;
    case NRSC5HIP_TUNE_HOST_CAPTURE: {
        if (e->hc_stream >= 0) { int rc = hc_detach(e); if (rc) return rc; }
        if (!e->hc_pin) break;                                 // window-pipeline engines have no fast seam
        e->host_capture = value != 0;
        if (value >= 512) {                                    // that many KiB of pinned capture instead of the default 16 MiB (tests: small values exercise hc_rebase)
            uint8_t *np = nullptr; void *dp = nullptr;
            if (hipHostMalloc((void **)&np, (size_t)value << 10, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dp, np, 0) != hipSuccess) FAIL(NRSC5HIP_ENOMEM, "pinned capture allocation failed");
            (void)hipHostFree(e->hc_pin);
            e->hc_pin = np; e->hc_dev = (uint8_t *)dp; e->hc_cap = (size_t)value << 10;
        }
        break;
    }
    case NRSC5HIP_TUNE_MIXFFT_SYMS: {
        e->mixfft_syms = (value == 2 || value == 4 || value == 8 || value == 16 || value == 32 || (value >= 100 && value <= 140)) ? value : 1;
        if (e->mixfft_syms >= 100) {                           // DIAGNOSTIC LDS padding: never beyond what a workgroup may have beside the kernel's own ~20 KB (an oversized request failed the
            int lds_max = 65536;                               // launch, and the failure surfaced at some later hipGetLastError)
#ifndef HIPEMU
            HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device));
#endif
            const int room_kib = (lds_max - 24 * 1024) / 1024;
            if (e->mixfft_syms - 100 > room_kib) e->mixfft_syms = 100 + std::max(room_kib, 0);
        }
        break;
    }
    case NRSC5HIP_TUNE_AM_SEGMENTS:       e->am_segments = std::min(std::max(value, 1), K9_GMAX); break;
    case NRSC5HIP_TUNE_AM_WARM:           e->am_warm = value > 0 ? K9_WARM : 0; e->am_runin = value > 0 ? K9_TB_RUNIN : 0; break;
    case NRSC5HIP_TUNE_SYNC_PHASES:
        if (value && !e->sync_phase_buf) {
            int rc = dev_alloc(e, &e->sync_phase_buf, 16); if (rc) return rc;
            HIPCHK(hipMemset(e->sync_phase_buf, 0, 16 * sizeof(long long)));
        }
        e->db.sync_phase_cycles = value ? e->sync_phase_buf : nullptr;
        break;
    default: FAIL(NRSC5HIP_EINVAL, "unknown knob %d", knob);
    }
    return 0;
}

extern "C" int nrsc5hip_debug_flow_stats(nrsc5hip_engine *e, long long stats[2])
{
    if (!e || !stats) return NRSC5HIP_EINVAL;
    stats[0] = e->flow_bursts; stats[1] = e->flow_steps;
    return 0;
}

extern "C" int nrsc5hip_debug_host_capture_stats(nrsc5hip_engine *e, long long stats[5])
{
    if (!e || !stats) return NRSC5HIP_EINVAL;
    stats[0] = e->hc_attaches; stats[1] = e->hc_detaches; stats[2] = e->hc_rebases; stats[3] = e->hc_stream; stats[4] = e->reports_folded;
    return 0;
}

extern "C" int nrsc5hip_debug_fwd_stats(nrsc5hip_engine *e, int stats[2])
{
    ON_ENGINE_DEVICE(e);
    if (!e || !stats) FAIL(NRSC5HIP_EINVAL, "null argument");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(stats, e->db.fwd_stats, 2 * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_debug_tb_stats(nrsc5hip_engine *e, int stats[2])
{
    ON_ENGINE_DEVICE(e);
    if (!stats) FAIL(NRSC5HIP_EINVAL, "null argument");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(stats, e->db.tb_stats, 2 * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_debug_k9_stats(nrsc5hip_engine *e, int stats[4])
{
    ON_ENGINE_DEVICE(e);
    if (!e || !stats) FAIL(NRSC5HIP_EINVAL, "null argument");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(stats, e->db.am_k9stats, 4 * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_debug_sync_phases(nrsc5hip_engine *e, long long *cycles16)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !cycles16) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (!e->sync_phase_buf) FAIL(NRSC5HIP_EINVAL, "turn the instrumentation on first: nrsc5hip_debug_tune(e, NRSC5HIP_TUNE_SYNC_PHASES, 1)");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(cycles16, e->sync_phase_buf, 16 * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}
