// The batch API: appends, the trim, batch_process and every fetch path that reads the device rings (records, frame bits, the L2
// audio transport index).  These move a stream's FIFO without the host mirror of the fast streaming seam (leave_mirror).
#include <algorithm>
#include "engine_internal.h"
// ---- batch path ----------------------------------------------------------------------------------------------
// the batch entry points move a stream's FIFO without the host mirror of the fast streaming seam: records are read from the device again
int nrsc5::leave_mirror(nrsc5hip_engine *e, int n, const int *ids)
{
    for (int k = 0; k < n; k++) if (e->hc_stream >= 0 && stream_at(ids, k) == e->hc_stream) { int rc = hc_detach(e); if (rc) return rc; }   // the batch kernels read a FIFO (or a capture of known length)
    if (e->staged_stream >= 0) { int rc = flush_staged(e); if (rc) return rc; }   // whatever a push left in the pinned buffer goes to the FIFO first
    for (int k = 0; k < n; k++) {
        const int s = stream_at(ids, k);
        if (s < 0 || s >= e->cfg.max_streams || !e->mirror_ok[s]) continue;
        e->mirror_ok[s] = 0; e->pending[s].clear(); e->fetched[s] = e->drained[s];
        forget_prediction(e, s);
    }
    e->counters_clean = false;
    return 0;
}

// a stream list in range: 1..max_streams entries, every id a stream of the engine (ids = nullptr: the identity list 0..n-1)
static int check_ids(const nrsc5hip_engine *e, int n, const int *ids)
{
    if (n < 1 || n > e->cfg.max_streams) FAIL(NRSC5HIP_EINVAL, "nstreams %d out of range", n);
    if (ids) for (int k = 0; k < n; k++) if (ids[k] < 0 || ids[k] >= e->cfg.max_streams) FAIL(NRSC5HIP_EINVAL, "stream id %d out of range", ids[k]);
    return 0;
}

int nrsc5::upload_ids(nrsc5hip_engine *e, int n, const int *ids, const uint32_t *counts, const int **ids_dev)
{
    int rc = check_ids(e, n, ids); if (rc) return rc;
    if (ids) {
        HIPCHK(hipMemcpy(e->ids_dev, ids, n * sizeof(int), hipMemcpyHostToDevice));
        *ids_dev = e->ids_dev;
    } else {
        // the identity set: every kernel resolves `ids ? ids[i] : i` (stream_of), and without the list the stream index costs no trip to memory in
        // front of the stream-state loads that depend on it (k_mixfft / k_sync begin with exactly that chain)
        *ids_dev = nullptr;
    }
    if (counts) HIPCHK(hipMemcpy(e->nbytes_dev, counts, n * sizeof(unsigned), hipMemcpyHostToDevice));
    return 0;
}

// an append that does not fit is refused whole (nothing is written, no counter moves); the appends never trim by themselves
static int fifo_overflow(nrsc5hip_engine *e, int s, long long incoming)
{
    FAIL(NRSC5HIP_EOVERFLOW, "stream %d: q15_capacity %lld too small for this batch: %lld samples retained + %lld appended (nrsc5hip_batch_trim gives back what nothing can read again)",
         s, e->db.q15_cap, e->wr_host[s] - e->base_host[s], incoming);
}

extern "C" int nrsc5hip_batch_append_cu8(nrsc5hip_engine *e, int nstreams, const int *stream_ids,
                                         const uint8_t *dev_iq, long long stride_bytes, const uint32_t *nbytes)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !dev_iq || !nbytes) FAIL(NRSC5HIP_EINVAL, "null argument");
    const int *ids_dev; int rc = upload_ids(e, nstreams, stream_ids, nbytes, &ids_dev); if (rc) return rc;
    if ((rc = leave_mirror(e, nstreams, stream_ids))) return rc;
    unsigned mx = 0;
    {
        int nam = 0;
        for (int k = 0; k < nstreams; k++) nam += e->mode_host[stream_at(stream_ids, k)] == MODE_AM;
        if (nam && nam != nstreams) FAIL(NRSC5HIP_EINVAL, "one append call must list streams of one mode (FM or AM)");
        if (nam) {
            for (int k = 0; k < nstreams; k++) {
                const int s = stream_at(stream_ids, k);
                if (nbytes[k] % 4) FAIL(NRSC5HIP_EINVAL, "chunk %d: nbytes %% 4 != 0", k);
                const long long nout = (e->raw_host[s] + nbytes[k] / 2) / 32 - e->raw_host[s] / 32;
                if (e->wr_host[s] - e->base_host[s] + nout > e->db.q15_cap) return fifo_overflow(e, s, nout);
                if (nbytes[k] > mx) mx = nbytes[k];
            }
            { ProfScope p(e, NRSC5HIP_PROF_DECIMATE, e->main); launch_am_decimate_cu8(e->tb, e->db, nstreams, ids_dev, dev_iq, stride_bytes, e->nbytes_dev, mx, e->main); }
            for (int k = 0; k < nstreams; k++) {
                const int s = stream_at(stream_ids, k);
                e->wr_host[s] += (e->raw_host[s] + nbytes[k] / 2) / 32 - e->raw_host[s] / 32;
                e->raw_host[s] += nbytes[k] / 2;
            }
            HIPCHK(hipGetLastError());
            return 0;
        }
    }
    for (int k = 0; k < nstreams; k++) {
        const int s = stream_at(stream_ids, k);
        if (e->attached[s]) FAIL(NRSC5HIP_EINVAL, "stream %d already reads a zero-copy capture (one append per reset)", s);
    }
    if (e->cfg.batch_zero_copy) {
        bool all_fresh = true;
        for (int k = 0; k < nstreams; k++) all_fresh = all_fresh && e->wr_host[stream_at(stream_ids, k)] == 0;
        if (all_fresh) {
            // zero-copy: the capture stays where it is; the block steps decimate what they read (k_mixfft, k_acq_decimate)
            if (((uintptr_t)dev_iq | (uintptr_t)stride_bytes) & 3) FAIL(NRSC5HIP_EINVAL, "zero-copy captures must be 4-byte aligned");
            for (int k = 0; k < nstreams; k++) if (nbytes[k] % 4) FAIL(NRSC5HIP_EINVAL, "chunk %d: nbytes %% 4 != 0", k);
            launch_attach_raw(e->db, nstreams, ids_dev, dev_iq, stride_bytes, e->nbytes_dev, e->main);
            for (int k = 0; k < nstreams; k++) { const int s = stream_at(stream_ids, k); e->wr_host[s] += nbytes[k] / 4; e->attached[s] = 1; }
            HIPCHK(hipGetLastError());
            return 0;
        }
    }
    for (int k = 0; k < nstreams; k++) {
        const int s = stream_at(stream_ids, k);
        if (nbytes[k] % 4) FAIL(NRSC5HIP_EINVAL, "chunk %d: nbytes %% 4 != 0", k);
        if (e->wr_host[s] - e->base_host[s] + nbytes[k] / 4 > e->db.q15_cap) return fifo_overflow(e, s, nbytes[k] / 4);
        if (nbytes[k] > mx) mx = nbytes[k];
    }
    bool fresh = e->cfg.p1_async != 0 && stream_ids == nullptr && nstreams == e->cfg.max_streams;
    for (int k = 0; k < nstreams && fresh; k++) fresh = e->wr_host[k] == 0;
    fresh = fresh && e->step_count == 0;
    const long long CH = 16 * 70199LL;                         // one decode window's worth of output samples
    if (fresh && (long long)mx / 4 > 3 * CH) {
        // Fresh batch in the pipelined mode: decimate window-sized chunks on a side stream so that K1 (HBM-bound)
        // overlaps the issue-bound block steps; the scheduler waits for the chunk a step can reach (issue_step, block_step.h).
        const int nch = (int)(((long long)mx / 4 + CH - 1) / CH);
        if (e->chunk_cap < nch * nstreams) {
            unsigned *p = nullptr;
            if (dev_alloc(e, &p, (size_t)nch * nstreams)) return NRSC5HIP_ENOMEM;
            e->chunk_nbytes_dev = p; e->chunk_cap = nch * nstreams;
        }
        std::vector<unsigned> cb((size_t)nch * nstreams);
        for (int c = 0; c < nch; c++)
            for (int k = 0; k < nstreams; k++) {
                const long long lo = 4 * CH * c, left = (long long)nbytes[k] - lo;
                cb[(size_t)c * nstreams + k] = (unsigned)(left <= 0 ? 0 : (left > 4 * CH ? 4 * CH : left));
            }
        HIPCHK(hipMemcpy(e->chunk_nbytes_dev, cb.data(), cb.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        while ((int)e->dec_events.size() < nch) { hipEvent_t ev; HIPCHK(hipEventCreate(&ev)); e->dec_events.push_back(ev); }
        hipEvent_t start; HIPCHK(hipEventCreate(&start));
        HIPCHK(hipEventRecord(start, e->main));                // after whatever the caller/engine queued before (reset)
        HIPCHK(hipStreamWaitEvent(e->dec_stream, start, 0));
        (void)hipEventDestroy(start);
        for (int c = 0; c < nch; c++) {
            ProfScope p(e, NRSC5HIP_PROF_DECIMATE, e->dec_stream);
            launch_decimate_fm_cu8(e->tb, e->db, nstreams, ids_dev, dev_iq + 4 * CH * c, stride_bytes,
                                   e->chunk_nbytes_dev + (size_t)c * nstreams, (unsigned)(4 * CH), e->dec_stream);
            HIPCHK(hipEventRecord(e->dec_events[c], e->dec_stream));
        }
        e->dec_chunk = CH;
        e->dec_waited = 0;
    } else {
        ProfScope p(e, NRSC5HIP_PROF_DECIMATE, e->main);
        launch_decimate_fm_cu8(e->tb, e->db, nstreams, ids_dev, dev_iq, stride_bytes, e->nbytes_dev, mx, e->main);
    }
    for (int k = 0; k < nstreams; k++) e->wr_host[stream_at(stream_ids, k)] += nbytes[k] / 4;
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nrsc5hip_batch_append_cs16(nrsc5hip_engine *e, int nstreams, const int *stream_ids,
                                          const int16_t *dev_iq, long long stride_elems, const uint32_t *nelems)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !dev_iq || !nelems) FAIL(NRSC5HIP_EINVAL, "null argument");
    const int *ids_dev; int rc = upload_ids(e, nstreams, stream_ids, nelems, &ids_dev); if (rc) return rc;
    if ((rc = leave_mirror(e, nstreams, stream_ids))) return rc;
    unsigned mx = 0;
    for (int k = 0; k < nstreams; k++) {
        const int s = stream_at(stream_ids, k);
        if (nelems[k] % 2) FAIL(NRSC5HIP_EINVAL, "chunk %d: odd cs16 length", k);
        if (e->attached[s]) FAIL(NRSC5HIP_EINVAL, "stream %d reads a zero-copy capture: reset it before appending samples", s);
        if (e->wr_host[s] - e->base_host[s] + nelems[k] / 2 > e->db.q15_cap) return fifo_overflow(e, s, nelems[k] / 2);
        if (nelems[k] > mx) mx = nelems[k];
    }
    launch_append_cs16(e->db, nstreams, ids_dev, dev_iq, stride_elems, e->nbytes_dev, mx, e->main);
    for (int k = 0; k < nstreams; k++) e->wr_host[stream_at(stream_ids, k)] += nelems[k] / 2;
    HIPCHK(hipGetLastError());
    return 0;
}


// Give back the slab space of the listed streams in front of everything that may still be read (k_trim.hip).  On the chain stream, the only consumer of
// db.q15, behind every block step and rollback submitted so far and ahead of the next append: batch_process returns with all of them done; ON_ENGINE_DEVICE
// runs settle(), which harvests a block step of the streaming seam that is still in flight and waits for the ingest stream; leave_mirror submits what a push
// left staged; a chunked append on the decimation stream is waited for here.
static_assert(NRSC5HIP_TRIM_RETAIN_MAX == (16LL * NWIN + 1) * WIN_N, "include/nrsc5hip.h states the retention bound of the pipeline depth");
static_assert(NRSC5HIP_TRIM_RETAIN_MAX_AM == (8LL * NWIN + 1) * AM_WIN, "include/nrsc5hip.h states the retention bound of the AM pipeline depth");
extern "C" int nrsc5hip_batch_trim(nrsc5hip_engine *e, int nstreams, const int *stream_ids, long long *retained)
{
    ON_ENGINE_DEVICE(e);
    if (!e) FAIL(NRSC5HIP_EINVAL, "null engine");
    int rc = check_ids(e, nstreams, stream_ids); if (rc) return rc;
    if (stream_ids) {
        std::vector<char> seen(e->cfg.max_streams, 0);         // a stream listed twice would be moved by two grid rows at once
        for (int k = 0; k < nstreams; k++) {
            if (seen[stream_ids[k]]) FAIL(NRSC5HIP_EINVAL, "stream id %d listed twice", stream_ids[k]);
            seen[stream_ids[k]] = 1;
        }
    }
    // streams that read a capture in place (zero-copy batch, the pinned host capture of the fast seam) hold nothing in the slab: left alone
    std::vector<int> act;
    for (int k = 0; k < nstreams; k++) {
        const int s = stream_at(stream_ids, k);
        if (retained) retained[k] = 0;
        if (!e->attached[s] && e->hc_stream != s) act.push_back(s);
    }
    if (act.empty()) return 0;
    const int n = (int)act.size();
    if ((rc = leave_mirror(e, n, act.data()))) return rc;
    if (e->dec_chunk) HIPCHK(hipStreamSynchronize(e->dec_stream));           // a chunked append still writing the slab
    HIPCHK(hipMemcpy(e->ids_dev, act.data(), n * sizeof(int), hipMemcpyHostToDevice));
    // workgroups per stream of the disjoint move: about 512 over the whole launch (two per CU), at most 32 per stream -- what is moved is under one window
    // (70 tiles of 4096 samples) per stream when the blocks have been processed.  Not tuned: a whole trim of 64 stations measured 0.1 ms.
    launch_trim(e->db, n, e->ids_dev, e->trim_plan_dev, std::min(32, std::max(1, 512 / n)), e->main);
    HIPCHK(hipGetLastError());
    std::vector<TrimPlan> plan(n);
    HIPCHK(hipMemcpyAsync(plan.data(), e->trim_plan_dev, n * sizeof(TrimPlan), hipMemcpyDeviceToHost, e->main));
    HIPCHK(hipStreamSynchronize(e->main));
    for (int k = 0; k < n; k++) {
        const int s = act[k];
        if (plan[k].wr != e->wr_host[s] || plan[k].base < e->base_host[s] || plan[k].base > plan[k].wr)
            FAIL(NRSC5HIP_EHIP, "stream %d: the trim found wr %lld base %lld where the host holds wr %lld base %lld", s, plan[k].wr, plan[k].base, e->wr_host[s], e->base_host[s]);
        e->base_host[s] = plan[k].base;
    }
    if (retained) for (int k = 0; k < nstreams; k++) {
        const int s = stream_at(stream_ids, k);
        if (!e->attached[s] && e->hc_stream != s) retained[k] = e->wr_host[s] - e->base_host[s];
    }
    return 0;
}

extern "C" int nrsc5hip_batch_process(nrsc5hip_engine *e, int nstreams, const int *stream_ids, int max_steps, int *steps_done)
{
    ON_ENGINE_DEVICE(e);
    if (!e) FAIL(NRSC5HIP_EINVAL, "null engine");
    int rc = check_ids(e, nstreams, stream_ids); if (rc) return rc;
    if ((rc = leave_mirror(e, nstreams, stream_ids))) return rc;
    {   // AM streams advance through their own fused block kernel; split a mixed list by mode
        std::vector<int> fm, am;
        for (int k = 0; k < nstreams; k++) { const int s = stream_at(stream_ids, k); (e->mode_host[s] == MODE_AM ? am : fm).push_back(s); }
        if (!am.empty()) {
            int done_am = 0, done_fm = 0;
            HIPCHK(hipMemcpy(e->ids_dev, am.data(), am.size() * sizeof(int), hipMemcpyHostToDevice));
            if ((rc = run_steps_am(e, (int)am.size(), e->ids_dev, max_steps > 0 ? max_steps : (1 << 30), e->cfg.p1_async ? 32 : 8, &done_am))) return rc;
            if (!fm.empty()) { rc = nrsc5hip_batch_process(e, (int)fm.size(), fm.data(), max_steps, &done_fm); if (rc) return rc; }
            if (steps_done) *steps_done = done_am > done_fm ? done_am : done_fm;
            return 0;
        }
    }
    const int *ids_dev; if ((rc = upload_ids(e, nstreams, stream_ids, nullptr, &ids_dev))) return rc;
    return run_steps(e, nstreams, ids_dev, set_signature(nstreams, stream_ids), max_steps > 0 ? max_steps : (1 << 30), e->cfg.p1_async ? 16 : 8, steps_done);
}

// ---- results ------------------------------------------------------------------------------------------------------
// Window pipeline, AM: the BER of an L1 frame is known when the last of its nine deferred decodes finishes, after the
// record of its block 7 was written -- it is kept per ring slot and merged into the records handed to the caller.
int nrsc5::patch_am_ber(nrsc5hip_engine *e, int stream, nrsc5hip_record *recs, int n, const float *ber_row)
{
    std::vector<float> tmp;
    if (!ber_row) {
        tmp.resize(e->db.p1_slots);
        HIPCHK(hipMemcpy(tmp.data(), e->db.am_ber + (size_t)stream * e->db.p1_slots, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
        ber_row = tmp.data();
    }
    for (int k = 0; k < n; k++)
        if ((recs[k].flags & NRSC5HIP_REC_P1) && recs[k].bc_decoded == 7 && recs[k].p1_slot >= 0 && recs[k].p1_slot < e->db.p1_slots)
            recs[k].ber = ber_row[recs[k].p1_slot];
    return 0;
}

extern "C" void nrsc5hip_unpack_bits(const uint32_t *words, int nbits, uint8_t *bits)
{
    // one byte of packed bits -> eight bytes through a table (a P1 frame is 146 176 bits: bit by bit this was ~0.1 ms of the drop-in's
    // host time per frame)
    static const struct Lut { uint64_t v[256]; Lut() { for (int b = 0; b < 256; b++) { uint64_t x = 0; for (int k = 0; k < 8; k++) x |= (uint64_t)((b >> k) & 1) << (8 * k); v[b] = x; } } } lut;
    const uint8_t *src = (const uint8_t *)words;               // little-endian host: bit i of the frame = bit i % 8 of byte i / 8
    int i = 0;
    for (; i + 8 <= nbits; i += 8) memcpy(bits + i, &lut.v[src[i >> 3]], 8);
    for (; i < nbits; i++) bits[i] = (words[i >> 5] >> (i & 31)) & 1u;
}

extern "C" int nrsc5hip_p1_frame_bits(nrsc5hip_engine *e, int stream, int slot, uint8_t *bits)
{
    ON_ENGINE_DEVICE_FAST(e);
    std::vector<uint32_t> w(P1_WORDS);
    int rc = nrsc5hip_p1_frame_packed(e, stream, slot, w.data()); if (rc) return rc;
    nrsc5hip_unpack_bits(w.data(), P1_LEN, bits);
    return 0;
}

// FM extended sidebands: P3 (channel 0) / P4 (channel 1) frame of a REC_P3 / REC_P4 record; slot = record.sis
extern "C" int nrsc5hip_px_frame_bits(nrsc5hip_engine *e, int stream, int slot, int channel, int nbits, uint8_t *bits)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (slot < 0 || slot >= e->db.px_slots || channel < 0 || channel > 1 || !bits || (nbits != 2304 && nbits != 4608)) FAIL(NRSC5HIP_EINVAL, "bad slot/argument");
    uint32_t w[PX_WORDS];
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(w, e->db.px_ring + (((size_t)stream * e->db.px_slots + slot) * 2 + channel) * PX_WORDS, (nbits / 32) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    nrsc5hip_unpack_bits(w, nbits, bits);
    return 0;
}

// bulk variant: all P3/P4 slots of the listed streams, [nstreams][8 * p1_slots][2][144] words
extern "C" int nrsc5hip_batch_fetch_px(nrsc5hip_engine *e, int nstreams, const int *stream_ids, uint32_t *frames)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !frames) FAIL(NRSC5HIP_EINVAL, "null argument");
    HIPCHK(hipDeviceSynchronize());
    const size_t per = (size_t)e->db.px_slots * 2 * PX_WORDS;
    for (int k = 0; k < nstreams; k++) {
        const int s = stream_at(stream_ids, k);
        int rc = check_stream(e, s); if (rc) return rc;
        HIPCHK(hipMemcpy(frames + (size_t)k * per, e->db.px_ring + (size_t)s * per, per * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

// AM: frames of one L1 frame share a ring slot: P1 frame of block b at word b * 118, the P3 frame at word 944
extern "C" int nrsc5hip_am_frame_bits(nrsc5hip_engine *e, int stream, int slot, int which, int nbits, uint8_t *bits)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (slot < 0 || slot >= e->db.p1_slots || !bits || which < 0 || which > 8) FAIL(NRSC5HIP_EINVAL, "bad slot/argument");
    const int maxbits = which < 8 ? AM_P1_LEN : AM_P3_LEN_MA3;
    if (nbits < 1 || nbits > maxbits) FAIL(NRSC5HIP_EINVAL, "nbits %d out of range", nbits);
    const int word0 = which < 8 ? which * AM_P1_WORDS : AM_P3_WORD0, words = (nbits + 31) / 32;
    std::vector<uint32_t> w(words);
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(w.data(), e->db.p1_ring + ((size_t)stream * e->db.p1_slots + slot) * P1_WORDS + word0, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    nrsc5hip_unpack_bits(w.data(), nbits, bits);
    return 0;
}

// ---- L2 audio transport index ---------------------------------------------------------------------------------------

// the device half: the job list goes up and the index kernel is queued on the chain stream; frames [n] and bytes [n][stride] (may be null) are DEVICE
// buffers and stay there -- nothing is waited for, nothing comes back (nrsc5hip_psd_feed reads them with its own kernel)
int nrsc5::l2_launch(nrsc5hip_engine *e, const std::vector<L2Job> &jobs, L2Job *djobs, nrsc5hip_l2_frame *dframes, uint8_t *dbytes, long long stride)
{
    const int n = (int)jobs.size();
    if (dbytes && stride < L2_MAX_BYTES) {
        for (const L2Job &j : jobs) if ((j.nbits - 22) / 8 > stride) FAIL(NRSC5HIP_EINVAL, "stride %lld too small for a %d-bit frame", stride, j.nbits);
    }
    HIPCHK(hipMemcpy(djobs, jobs.data(), sizeof(L2Job) * n, hipMemcpyHostToDevice));
    launch_l2_index(djobs, n, dframes, dbytes, stride, e->main);
    HIPCHK(hipGetLastError());
    return 0;
}

int nrsc5::l2_run(nrsc5hip_engine *e, const std::vector<L2Job> &jobs, nrsc5hip_l2_frame *out, uint8_t *pdu_bytes, long long stride)
{
    const int n = (int)jobs.size();
    DevTmp tj, to, tb;                                  // freed on every return path
    HIPCHK(hipMalloc(&tj.p, sizeof(L2Job) * n));
    HIPCHK(hipMalloc(&to.p, sizeof(nrsc5hip_l2_frame) * n));
    if (pdu_bytes) HIPCHK(hipMalloc(&tb.p, (size_t)stride * n));
    nrsc5hip_l2_frame *dout = (nrsc5hip_l2_frame *)to.p; uint8_t *dbytes = (uint8_t *)tb.p;
    int rc = l2_launch(e, jobs, (L2Job *)tj.p, dout, dbytes, stride); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(out, dout, sizeof(nrsc5hip_l2_frame) * n, hipMemcpyDeviceToHost));
    if (pdu_bytes) HIPCHK(hipMemcpy(pdu_bytes, dbytes, (size_t)stride * n, hipMemcpyDeviceToHost));
    return 0;
}

// every slot / channel / length the jobs name, checked against the engine's rings; -> the frames' words in device memory
int nrsc5::l2_resolve(nrsc5hip_engine *e, int njobs, const nrsc5hip_l2_job *jobs, std::vector<L2Job> &dj)
{
    dj.resize((size_t)njobs);
    for (int k = 0; k < njobs; k++) {
        const nrsc5hip_l2_job &j = jobs[k];
        int rc = check_stream(e, j.stream); if (rc) return rc;
        const uint32_t *words = nullptr;
        if (j.kind == NRSC5HIP_L2_FM_P1) {
            if (j.slot < 0 || j.slot >= e->db.p1_slots || j.nbits != P1_LEN) FAIL(NRSC5HIP_EINVAL, "job %d: bad P1 slot / length", k);
            words = e->db.p1_ring + ((size_t)j.stream * e->db.p1_slots + j.slot) * P1_WORDS;
        } else if (j.kind == NRSC5HIP_L2_FM_PX) {
            if (j.slot < 0 || j.slot >= e->db.px_slots || j.which < 0 || j.which > 1 || (j.nbits != 2304 && j.nbits != 4608)) FAIL(NRSC5HIP_EINVAL, "job %d: bad P3/P4 slot / channel / length", k);
            words = e->db.px_ring + (((size_t)j.stream * e->db.px_slots + j.slot) * 2 + j.which) * PX_WORDS;
        } else if (j.kind == NRSC5HIP_L2_AM) {
            const bool p1 = j.which >= 0 && j.which < 8 && j.nbits == AM_P1_LEN;
            const bool p3 = j.which == 8 && (j.nbits == AM_P3_LEN_MA1 || j.nbits == AM_P3_LEN_MA3);
            if (j.slot < 0 || j.slot >= e->db.p1_slots || !(p1 || p3)) FAIL(NRSC5HIP_EINVAL, "job %d: bad AM slot / frame / length", k);
            words = e->db.p1_ring + ((size_t)j.stream * e->db.p1_slots + j.slot) * P1_WORDS + (p1 ? j.which * AM_P1_WORDS : AM_P3_WORD0);
        } else FAIL(NRSC5HIP_EINVAL, "job %d: unknown kind %d", k, j.kind);
        dj[k] = L2Job{words, j.nbits, 0};
    }
    return 0;
}

extern "C" int nrsc5hip_l2_index(nrsc5hip_engine *e, int njobs, const nrsc5hip_l2_job *jobs, nrsc5hip_l2_frame *out, uint8_t *pdu_bytes, long long stride)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !jobs || !out || njobs < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    std::vector<L2Job> dj;
    int rc = l2_resolve(e, njobs, jobs, dj); if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());                 // the frames may still be in flight on a decode stream
    return l2_run(e, dj, out, pdu_bytes, stride);
}

extern "C" int nrsc5hip_l2_frame_get(nrsc5hip_engine *e, int stream, int slot, nrsc5hip_l2_frame *out)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (!e->db.l2_ring) FAIL(NRSC5HIP_EINVAL, "engine was created without l2_index");
    if (slot < 0 || slot >= e->db.p1_slots || !out) FAIL(NRSC5HIP_EINVAL, "bad slot/argument");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, e->db.l2_ring + (size_t)stream * e->db.p1_slots + slot, sizeof(*out), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_batch_fetch_l2(nrsc5hip_engine *e, int nstreams, const int *stream_ids, nrsc5hip_l2_frame *out)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !out || nstreams < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    if (!e->db.l2_ring) FAIL(NRSC5HIP_EINVAL, "engine was created without l2_index");
    HIPCHK(hipDeviceSynchronize());
    const size_t per = (size_t)e->db.p1_slots;
    bool contiguous = true;
    for (int k = 0; k < nstreams; k++) {
        const int s = stream_at(stream_ids, k);
        int rc = check_stream(e, s); if (rc) return rc;
        if (s != stream_at(stream_ids, 0) + k) contiguous = false;
    }
    if (contiguous) {
        HIPCHK(hipMemcpy(out, e->db.l2_ring + (size_t)stream_at(stream_ids, 0) * per, (size_t)nstreams * per * sizeof(*out), hipMemcpyDeviceToHost));
    } else {
        for (int k = 0; k < nstreams; k++)
            HIPCHK(hipMemcpy(out + (size_t)k * per, e->db.l2_ring + (size_t)stream_ids[k] * per, per * sizeof(*out), hipMemcpyDeviceToHost));
    }
    return 0;
}

static int fetch_l2_ring(nrsc5hip_engine *e, const nrsc5hip_l2_frame *ring, size_t per, int nstreams, const int *stream_ids, nrsc5hip_l2_frame *out, const char *what)
{
    if (!e || !out || nstreams < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    if (!ring) FAIL(NRSC5HIP_EINVAL, "engine was created without l2_index%s", what);
    HIPCHK(hipDeviceSynchronize());
    for (int k = 0; k < nstreams; k++) {
        const int s = stream_at(stream_ids, k);
        int rc = check_stream(e, s); if (rc) return rc;
        HIPCHK(hipMemcpy(out + (size_t)k * per, ring + (size_t)s * per, per * sizeof(*out), hipMemcpyDeviceToHost));
    }
    return 0;
}
extern "C" int nrsc5hip_batch_fetch_l2_px(nrsc5hip_engine *e, int nstreams, const int *stream_ids, nrsc5hip_l2_frame *out)
{
    ON_ENGINE_DEVICE(e);
    return fetch_l2_ring(e, e ? e->db.l2_px_ring : nullptr, e ? (size_t)e->db.px_slots * 2 : 0, nstreams, stream_ids, out, "");
}
extern "C" int nrsc5hip_batch_fetch_l2_am(nrsc5hip_engine *e, int nstreams, const int *stream_ids, nrsc5hip_l2_frame *out)
{
    ON_ENGINE_DEVICE(e);
    return fetch_l2_ring(e, e ? e->db.l2_am_ring : nullptr, e ? (size_t)e->db.p1_slots * 9 : 0, nstreams, stream_ids, out, " and am_enable");
}
extern "C" int nrsc5hip_batch_fetch(nrsc5hip_engine *e, int nstreams, const int *stream_ids, nrsc5hip_record *records,
                                    int max_records, int *counts, uint32_t *frames)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !records || !counts) FAIL(NRSC5HIP_EINVAL, "null argument");
    HIPCHK(hipStreamSynchronize(e->main));
    for (int k = 0; k < nstreams; k++) {
        const int s = stream_at(stream_ids, k);
        int rc = check_stream(e, s); if (rc) return rc;
        int n = 0;
        rc = nrsc5hip_drain(e, s, records + (size_t)k * max_records, max_records, &n); if (rc) return rc;
        counts[k] = n;
        if (frames)
            HIPCHK(hipMemcpy(frames + (size_t)k * e->db.p1_slots * P1_WORDS, e->db.p1_ring + (size_t)s * e->db.p1_slots * P1_WORDS,
                             (size_t)e->db.p1_slots * P1_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

// Zero-copy variant of nrsc5hip_batch_fetch for streams 0..nstreams-1: three bulk D2H copies into engine-owned
// pinned buffers; the returned pointers stay valid until the next fetch/reset.  records: [nstreams][record_capacity],
// frames: [nstreams][p1_slots][4568].  Requires that nothing was drained since the last reset.
extern "C" int nrsc5hip_batch_fetch_view(nrsc5hip_engine *e, int nstreams, const nrsc5hip_record **records, int *counts, const uint32_t **frames)
{
    ON_ENGINE_DEVICE(e);
    if (!e || !records || !counts) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (nstreams < 1 || nstreams > e->cfg.max_streams) FAIL(NRSC5HIP_EINVAL, "nstreams out of range");
    { int rc = leave_mirror(e, nstreams, nullptr); if (rc) return rc; }
    const size_t S = e->cfg.max_streams;
    if (!e->rec_host) {
        HIPCHK(hipHostMalloc((void **)&e->rec_host, S * e->db.rec_cap * sizeof(BlockRecord), hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void **)&e->nblocks_host, S * sizeof(int), hipHostMallocDefault));
    }
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy2DAsync(e->nblocks_host, sizeof(int), (const char *)e->db.state + offsetof(StreamState, nblocks), sizeof(StreamState),
                            sizeof(int), nstreams, hipMemcpyDeviceToHost, e->main));
    HIPCHK(hipStreamSynchronize(e->main));
    int maxn = 0;
    bool any_am = false;
    for (int s = 0; s < nstreams; s++) { if (e->nblocks_host[s] > maxn) maxn = e->nblocks_host[s]; any_am |= e->mode_host[s] == MODE_AM; }
    if (maxn > e->db.rec_cap) maxn = e->db.rec_cap;
    // records: only the used head of every stream's ring (the view needs unwrapped rings anyway, checked below)
    if (maxn > 0)
        HIPCHK(hipMemcpy2DAsync(e->rec_host, (size_t)e->db.rec_cap * sizeof(BlockRecord), e->db.records, (size_t)e->db.rec_cap * sizeof(BlockRecord),
                                (size_t)maxn * sizeof(BlockRecord), nstreams, hipMemcpyDeviceToHost, e->main));
    if (frames) {
        // P1 frames: the first view copies the ring and hands the pinned buffer to the FM traceback as a mirror (DevBuffers::
        // p1_mirror); from then on every frame reaches the host while the pass is still running and nothing is left to copy here.
        // AM frames are written by other kernels: a batch with AM streams keeps copying.
        const size_t nwords = (size_t)e->db.p1_slots * P1_WORDS;
        if (!e->frames_host) {
            HIPCHK(hipHostMalloc((void **)&e->frames_host, S * nwords * sizeof(uint32_t), hipHostMallocMapped));
            HIPCHK(hipMemcpyAsync(e->frames_host, e->db.p1_ring, S * nwords * sizeof(uint32_t), hipMemcpyDeviceToHost, e->main));
            void *dp = nullptr;
            HIPCHK(hipHostGetDevicePointer(&dp, e->frames_host, 0));
            e->db.p1_mirror = (uint32_t *)dp;
        } else if (any_am) {
            HIPCHK(hipMemcpyAsync(e->frames_host, e->db.p1_ring, (size_t)nstreams * nwords * sizeof(uint32_t), hipMemcpyDeviceToHost, e->main));
        }
    }
    HIPCHK(hipStreamSynchronize(e->main));
    if (e->cfg.p1_async && e->db.am) {
        std::vector<float> ber((size_t)nstreams * e->db.p1_slots);
        bool any = false;
        for (int s = 0; s < nstreams; s++) any |= e->mode_host[s] == MODE_AM;
        if (any) {
            HIPCHK(hipMemcpy(ber.data(), e->db.am_ber, ber.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (int s = 0; s < nstreams; s++)
                if (e->mode_host[s] == MODE_AM) {
                    const int nrec = e->nblocks_host[s] < e->db.rec_cap ? e->nblocks_host[s] : e->db.rec_cap;
                    patch_am_ber(e, s, (nrsc5hip_record *)e->rec_host + (size_t)s * e->db.rec_cap, nrec, ber.data() + (size_t)s * e->db.p1_slots);
                }
        }
    }
    for (int s = 0; s < nstreams; s++) {
        if (e->drained[s] != 0 || e->nblocks_host[s] > e->db.rec_cap)
            FAIL(NRSC5HIP_EOVERFLOW, "stream %d: view needs an undrained, unwrapped record ring (%d records, capacity %d)", s, e->nblocks_host[s], e->db.rec_cap);
        int n = e->nblocks_host[s];
        e->drained[s] = n;
        if (e->db.ckpt || e->db.am_ckpt) {                     // replay: squeeze the void records out, in place in the pinned buffer
            BlockRecord *r = e->rec_host + (size_t)s * e->db.rec_cap;
            int m = 0;
            for (int k = 0; k < n; k++) if (!(r[k].flags & REC_DISCARDED)) { if (m != k) r[m] = r[k]; m++; }
            n = m;
        }
        counts[s] = n;
    }
    *records = (const nrsc5hip_record *)e->rec_host;
    if (frames) *frames = e->frames_host;
    return 0;
}
