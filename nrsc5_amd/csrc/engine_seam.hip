// The fast streaming seam (p1_async = 0): pushes staged in pinned memory or kept as a host-resident capture, one block step in flight
// with its report posted into pinned memory, the host mirror of the FIFO, drains.  Mirrors the reference's src/input.c seam
// (input_push_cu8/cs16) -- see include/nrsc5hip.h for the map.  ONE unit: the chain that runs once per push is static and inlinable.
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include "block_step.h"

// wall-clock totals of the fast streaming seam of the CALLING THREAD's sessions (nrsc5hip_debug_seam_totals): where a drop-in
// session's time goes.  Thread-local: sessions driven from different threads never share a counter.
__thread double nrsc5::g_seam[14];     // [0] s copying pushes into pinned staging, [1] s enqueueing H2D + decimator, [2] s enqueueing block steps,
                           // [3] s waiting for the device (the one sync per block), [4] pushes, [5] submissions, [6] block steps, [7] s in drain / frame fetches,
                           // [8] block steps whose wait was deferred, [9] read positions mispredicted, [10] steps without the P1 decode launches,
                           // [11] P1 decodes launched after the fact (the prediction said no frame could complete),
                           // [12] block steps submitted ahead of the previous block's delivery
struct SeamClock {
    int slot; std::chrono::steady_clock::time_point t0;
    explicit SeamClock(int s) : slot(s), t0(std::chrono::steady_clock::now()) {}
    ~SeamClock() { g_seam[slot] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

// ---- FIFO space management (streaming) -----------------------------------------------------------------
__global__ void k_compact(DevBuffers db, int s)
{
    // move the unread tail [rd, wr) to the start of the stream's slab; forward copy, dst < src
    StreamState &st = db.state[s];
    c16 *buf = db.q15 + (size_t)s * db.q15_cap;
    const long long off = st.rd - st.base, n = st.wr - st.rd;
    __shared__ c16 tmp[1024];
    for (long long c = 0; c < n; c += 1024) {
        const long long k = c + threadIdx.x;
        if (k < n) tmp[threadIdx.x] = buf[off + k];
        __syncthreads();
        if (k < n) buf[k] = tmp[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) st.base = st.rd;
}

static int ensure_space(nrsc5hip_engine *e, int s, long long incoming, bool on_ingest = false)
{
    if (e->wr_host[s] - e->base_host[s] + incoming <= e->db.q15_cap) return 0;
    if (on_ingest && e->main_stepped) {                        // the compaction moves [rd, wr): the steps submitted so far must have left their final rd
        HIPCHK(hipEventRecord(e->ev_main, e->main));
        HIPCHK(hipStreamWaitEvent(e->ingest, e->ev_main, 0));
        e->main_stepped = false;
    }
    hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, on_ingest ? e->ingest : e->main, e->db, s);
    if (e->mirror_ok[s]) {
        e->base_host[s] = e->rd_host[s];                       // k_compact sets base = rd, and the mirror IS the device's rd
    } else {
        long long base = 0;
        HIPCHK(hipMemcpyAsync(&base, (const char *)(e->db.state + s) + offsetof(StreamState, base), sizeof(long long), hipMemcpyDeviceToHost, e->main));
        HIPCHK(hipStreamSynchronize(e->main));
        e->base_host[s] = base;
    }
    if (e->wr_host[s] - e->base_host[s] + incoming > e->db.q15_cap)
        FAIL(NRSC5HIP_EOVERFLOW, "stream %d: FIFO capacity %lld too small for %lld more samples", s, e->db.q15_cap, incoming);
    return 0;
}

// ---- streaming seam ---------------------------------------------------------------------------------------
// (the report itself is the tail of the step's last kernel: k_stream_tail, k_pids_px.hip)
static int window_of(const nrsc5hip_engine *e, int s) { return e->mode_host[s] == MODE_AM ? AM_WIN : WIN_N; }


// Wait for the report with sequence number `seq`: the kernel's last store is that number into mapped pinned memory, so the
// host spins on it (a stream synchronisation returns ~5-10 us after the kernel has ended); bounded, then the ordinary wait.
static int wait_report(nrsc5hip_engine *e, unsigned seq, bool block)
{
    const volatile unsigned *p = &e->report_host[seq & 1]->seq;
    if (__atomic_load_n(p, __ATOMIC_ACQUIRE) == seq) return 1;
    if (!block) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int spins = 0;; spins++) {
        if (__atomic_load_n(p, __ATOMIC_ACQUIRE) == seq) return 1;
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;   // a block step is ~50 us: past 2 ms something else holds the queue -- stop burning a core, block
    }
    HIPCHK(hipStreamSynchronize(e->main));
    if (__atomic_load_n(p, __ATOMIC_ACQUIRE) != seq) FAIL(NRSC5HIP_EHIP, "stream report %u never arrived (have %u)", seq, *p);
    return 1;
}

// the next report's sequence number, buffer and first record
static StepReport next_report(nrsc5hip_engine *e, int s)
{
    e->report_seq++;
    if (e->report_seq == 0) e->report_seq = 2;                 // 0 = the freshly cleared report; 2, not 1: the step before the wrap posted into buffer 1 (seq & 1)
    // records to post: from the first one the host has not seen -- the block of a step still in flight is not this step's to report
    const int first_rec = e->fetched[s] + ((e->inflight_stream == s) ? 1 : 0);
    return StepReport{ e->report_dev[e->report_seq & 1], e->report_seq, first_rec, false };
}

static int launch_report(nrsc5hip_engine *e, int s, bool with_pids, const StepReport *prepared = nullptr)
{
    const StepReport r = prepared ? *prepared : next_report(e, s);
    launch_stream_tail(e->tb, e->db, s, r.first_rec, r.out, r.seq, with_pids ? 1 : 0, e->main);
    e->counters_clean = true;
    HIPCHK(hipGetLastError());
    return 0;
}

// Take the report of the step in flight (if any).  block = false: only if it has arrived.  Returns < 0 on error.
static int harvest(nrsc5hip_engine *e, bool block)
{
    const int s = e->inflight_stream;
    if (s < 0) return 0;
    {
        const auto t_wait = std::chrono::steady_clock::now();
        const int got = wait_report(e, e->inflight_seq, block);
        if (got < 0) return got;
        if (!got) return 0;
        if (block) g_seam[3] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wait).count();
    }
    e->inflight_stream = -1;
    const StreamReport *rp = e->report_host[e->inflight_seq & 1];
    bool p1_missing = false;
    for (int k = 0; k < rp->nrec; k++) if ((rp->rec[k].flags & REC_P1) && e->mode_host[s] != MODE_AM && !e->inflight_decoded) p1_missing = true;
    if (p1_missing) {
        // the prediction said no P1 frame could complete in this block and one did: decode it now, take the record again
        g_seam[11] += 1;
        if (e->ahead.valid) {
            // cannot happen while the caller keeps the contract of nrsc5hip_stream_step_ahead (nothing that changes L1 state between it and the drain);
            // if it does, leave the engine in a state every later call understands: nothing in flight, the stream's mirror invalid (its next push
            // re-synchronises with the device), then report.  What is LOST in this case, and documented as such (include/nrsc5hip.h, nrsc5hip_stream_step_ahead): the events
            // of the two blocks already run on the device are not delivered through the seam -- their records stay in the device ring and are visible to
            // nrsc5hip_drain / nrsc5hip_batch_fetch, but the frame of the first lacks its decode (no P1 bits, no BER); the caller's session is over (error return).
            e->ahead.valid = false; e->inflight_rd_pred = -1;
            (void)hipStreamSynchronize(e->main);
            e->mirror_ok[s] = 0; forget_prediction(e, s);
            FAIL(NRSC5HIP_EHIP, "stream %d: a block submitted without its P1 decode completed a frame, and the next block is already running", s);
        }
        int rc = launch_inorder_p1(e, 1, e->all_ids_dev + s); if (rc) return rc;
        if ((rc = launch_report(e, s, false))) return rc;
        if ((rc = wait_report(e, e->report_seq, true)) < 0) return rc;
        rp = e->report_host[e->report_seq & 1];
    }
    e->acq_needed = rp->counters[1] > 0;
    e->px_needed = rp->counters[2] > 0;
    if (e->inflight_rd_pred >= 0 && e->inflight_rd_pred != rp->rd) g_seam[9] += 1;      // never seen; the mirror is put right below
    e->rd_host[s] = rp->rd;
    for (int k = 0; k < rp->nrec; k++) e->pending[s].push_back(rp->rec[k]);
    e->fetched[s] += rp->nrec;
    if (rp->nblocks != e->fetched[s]) FAIL(NRSC5HIP_EOVERFLOW, "stream %d: %d records behind the report", s, rp->nblocks - e->fetched[s]);
    if (rp->nrec > 0) {
        const BlockRecord &r = rp->rec[rp->nrec - 1];
        e->pred_ok[s] = (r.state_after == SYNC_FINE && !(r.flags & REC_LOST_SYNC)) ? 1 : 0;
        e->pred_samperr[s] = r.next_samperr; e->pred_bc[s] = r.bc;
    }
    e->inflight_progress = rp->counters[0] != 0;
    if (e->ahead.valid) {
        // the step submitted ahead becomes the step in flight; now that its predecessor's record is here, so does its prediction
        const int s2 = e->ahead.stream;
        e->ahead.valid = false;
        e->inflight_stream = s2; e->inflight_seq = e->ahead.seq; e->inflight_decoded = e->ahead.decoded; e->inflight_rd_pred = -1;
        if (e->pred_ok[s2] && !e->cfg.l2_feedback && e->defer_wait) {
            e->inflight_rd_pred = e->rd_host[s2] + WIN_N - SYM_N + e->pred_samperr[s2];
            e->rd_host[s2] = e->inflight_rd_pred;
            g_seam[8] += 1;
        } else {
            return harvest(e, true);                           // not predictable after all: wait for it now
        }
        return 0;
    }
    if (e->prof_on) { HIPCHK(hipStreamSynchronize(e->main)); prof_collect(e); }
    return 0;
}

// Submit one block step of stream s (its window is complete by the mirror) and the report kernel behind it.
// ahead: a step of the same stream is still in flight (FINE at its start, no P1 decode): this one is queued behind it.
static int submit_step(nrsc5hip_engine *e, int s, bool ahead = false)
{
    const int *ids_dev = e->all_ids_dev + s;                   // identity list: entry s is s
    const bool am = e->mode_host[s] == MODE_AM;
    const unsigned long long sig = set_signature(1, &s);
    if (sig != e->set_sig) { e->acq_needed = true; e->px_needed = true; e->set_sig = sig; }
    e->prepared_by_sync = false;
    const auto t_enq = std::chrono::steady_clock::now();
    if (e->ingest_dirty) { HIPCHK(hipEventRecord(e->ev_ingest, e->ingest)); HIPCHK(hipStreamWaitEvent(e->main, e->ev_ingest, 0)); e->ingest_dirty = false; }
    e->main_stepped = true;
    if (!e->counters_clean) HIPCHK(hipMemsetAsync(e->db.counters, 0, 4 * sizeof(int), e->main));
    // A P1 frame completes only in a block that starts FINE with block count 15 (k_sync: started_pm && bc == 15; a block that
    // locks restarts the frame): when the stream's last record says otherwise the three decode launches are left out.
    const bool known = e->pred_ok[s] && !e->cfg.l2_feedback;
    bool decode = true, have_rep = false;
    StepReport rep{};
    if (am) {
        ProfScope p(e, NRSC5HIP_PROF_AM, e->main);
        launch_am_step(e->tb, e->db, 1, ids_dev, e->main, e->cfg.l2_feedback, -1, (int)(e->am_step_count % 8), (int)(e->am_step_count / 8));
        e->am_step_count++;
    } else {
        // (ahead: the block in flight runs FINE with block count pred_bc and ends no frame, so this one runs with pred_bc + 1)
        const int bc = ahead ? (e->pred_bc[s] + 1) % 16 : e->pred_bc[s];
        decode = !(known && bc != 15);
        if (!decode) g_seam[10] += 1;
        rep = next_report(e, s); have_rep = true;
        int rc = issue_step(e, 1, ids_dev, decode, false, known && e->fuse_seam_prepare, e->fold_report ? &rep : nullptr); if (rc) return rc;   // PIDS frame: inside k_sync (pids_inline)
    }
    if (have_rep && rep.folded) { e->counters_clean = true; e->reports_folded++; }        // k_sync posted it
    else { int rc = launch_report(e, s, false, have_rep ? &rep : nullptr); if (rc) return rc; }    // FM: the PIDS frame was decoded inside k_sync; AM: inside its block kernel
    g_seam[2] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_enq).count();
    g_seam[6] += 1;
    if (ahead) { e->ahead.valid = true; e->ahead.stream = s; e->ahead.seq = e->report_seq; e->ahead.decoded = decode; g_seam[12] += 1; return 0; }
    e->inflight_stream = s; e->inflight_decoded = decode; e->inflight_rd_pred = -1; e->inflight_seq = e->report_seq;
    if (!am && known && e->defer_wait) {
        // the block starts FINE: samperr = 1080 + the previous block's feedback, keep = 2160 + (1080 - samperr), no keep_extra
        // (acquire.c:112,259; k_sync's tail): the mirror moves now, the report is taken when somebody needs it
        e->inflight_rd_pred = e->rd_host[s] + WIN_N - SYM_N + e->pred_samperr[s];
        e->rd_host[s] = e->inflight_rd_pred;
        g_seam[8] += 1;
    }
    return 0;
}

// Fast seam: block steps of one stream while the host mirror says a window is complete.  A step whose outcome the mirror can
// predict stays in flight when this returns (harvest takes it); any other is waited for here, as before.
static int stream_steps(nrsc5hip_engine *e, int s)
{
    int guard = 0;
    while (e->wr_host[s] - e->rd_host[s] >= window_of(e, s)) {
        int rc = 0;
        while (e->inflight_stream >= 0) if ((rc = harvest(e, true))) return rc;     // nothing in flight when a step is submitted here
        if (e->wr_host[s] - e->rd_host[s] < window_of(e, s)) break;
        if ((rc = submit_step(e, s))) return rc;
        if (e->inflight_rd_pred >= 0) continue;                // deferred: the mirror already shows the block consumed
        if ((rc = harvest(e, true))) return rc;
        if (!e->inflight_progress || ++guard > 64) break;      // nothing was processed or is pending
    }
    return 0;
}

int nrsc5::settle(nrsc5hip_engine *e)
{
    if (!e) return 0;
    while (e->inflight_stream >= 0) { int rc = harvest(e, true); if (rc) return rc; }
    if (e->ingest_dirty) { HIPCHK(hipStreamSynchronize(e->ingest)); e->ingest_dirty = false; }    // whatever follows runs on `main` (or the host) alone
    return 0;
}

// how many input BYTES of this format complete the stream's next block (the drop-in pushes exactly that much, so that the L2
// feedback of the block's frames reaches the engine before the next block); -1: not known (the stream is not driven by the
// streaming seam alone, or p1_async)
extern "C" long long nrsc5hip_bytes_to_next_block(nrsc5hip_engine *e, int stream, int cu8)
{
    if (!e || stream < 0 || stream >= e->cfg.max_streams || !e->mirror_ok[stream]) return -1;
    if (e->ahead.valid) { DeviceGuard guard(e->cfg.device); if (harvest(e, true)) return -1; }     // the mirror lacks the step submitted ahead until its predecessor is harvested
    long long need = window_of(e, stream) - (e->wr_host[stream] - e->rd_host[stream]);     // decimated samples
    if (need < 1) need = 1;
    if (!cu8) return need * 4;                                                             // cs16: 4 bytes per complex sample
    if (e->mode_host[stream] != MODE_AM) return need * 4;                                  // FM cu8: 2 raw samples of 2 bytes each
    const long long raw = e->raw_host[stream];                                             // AM cu8: output k appears with raw sample 32 k + 31
    return 2 * ((raw / 32 + need) * 32 - raw);
}

// submit the staged samples of the fast seam: one async H2D from pinned memory ([count (u32), pad to 16][samples]) + the decimator
int nrsc5::flush_staged(nrsc5hip_engine *e)
{
    const int s = e->staged_stream;
    if (s < 0 || e->staged_bytes == 0) { e->staged_stream = -1; return 0; }
    SeamClock clk(1); g_seam[5] += 1;
    const int slot = e->stage_slot;
    const bool cu8 = e->staged_cu8, am = e->mode_host[s] == MODE_AM;
    const size_t chunk = e->staged_bytes;
    const unsigned count = cu8 ? (unsigned)chunk : (unsigned)(chunk / 2);
    e->staged_stream = -1; e->staged_bytes = 0; e->staged_q15 = 0;
    e->stage_slot = (slot + 1) % nrsc5hip_engine::NSTAGE;     // the next pushes fill the next buffer
    const bool direct = cu8 && !am && e->direct_decimate;
    // (measured, profiles/r04_dropin_timeline.txt: with the block's last chunk on the step stream instead -- no dependency across two
    // queues in front of the step -- the decimator's own ~11 us of PCIe round trips sit on the chain and the drop-in is slower, 870 x
    // against 990 x; every chunk of the direct decimator goes on the ingest stream)
    const bool on_ingest = direct;
    if (!on_ingest && e->ingest_dirty) {                       // the FIFO is appended to in submission order whichever stream does it
        HIPCHK(hipEventRecord(e->ev_ingest, e->ingest)); HIPCHK(hipStreamWaitEvent(e->main, e->ev_ingest, 0)); e->ingest_dirty = false;
    }
    if (on_ingest && e->main_appended) {                       // ... and the next block's first chunk goes behind this block's last
        HIPCHK(hipStreamWaitEvent(e->ingest, e->ev_appended, 0)); e->main_appended = false;   // (recorded right behind that chunk: not behind the step that followed it)
    }
    int rc = ensure_space(e, s, 0, on_ingest); if (rc) return rc; // wr_host already counts the staged samples
    memcpy(e->stage_pin[slot], &count, sizeof(count));
    hipStream_t used = e->main;
    if (direct) {
        // FM cu8: the decimator reads the pinned buffer itself (one launch: no copy, no commit kernel)
        if (on_ingest) { used = e->ingest; e->ingest_dirty = true; }
        launch_decimate_fm_cu8_stream(e->tb, e->db, s, e->stage_pin_dev[slot] + 16, count, e->decim_ticket, used);
    } else {
        HIPCHK(hipMemcpyAsync(e->stage_dev2[slot], e->stage_pin[slot], chunk + 16, hipMemcpyHostToDevice, e->main));
        const int *ids_dev = e->all_ids_dev + s; const unsigned *count_dev = (const unsigned *)e->stage_dev2[slot]; const uint8_t *data_dev = e->stage_dev2[slot] + 16;
        if (cu8 && am) launch_am_decimate_cu8(e->tb, e->db, 1, ids_dev, data_dev, 0, count_dev, count, e->main);
        else if (cu8) launch_decimate_fm_cu8(e->tb, e->db, 1, ids_dev, data_dev, 0, count_dev, count, e->main);
        else launch_append_cs16(e->db, 1, ids_dev, (const int16_t *)data_dev, 0, count_dev, count, e->main);
    }
    if (!on_ingest) { HIPCHK(hipEventRecord(e->ev_appended, e->main)); e->main_appended = true; }
    HIPCHK(hipEventRecord(e->stage_ev[slot], used)); e->stage_busy[slot] = true;
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- host-resident capture (see nrsc5hip_engine::hc_*) ------------------------------------------------------------
static int push_common(nrsc5hip_engine *e, int s, const void *host, size_t nbytes_total, bool cu8);

// complex input sample k of the bound stream's session (k >= -14: its decimator history) as the Q15 pair the reference's decimator holds (U8_Q15, defines.h:93)
static c16 hc_sample_q15(const nrsc5hip_engine *e, long long k)
{
    const uint8_t *b = e->hc_pin + (nrsc5hip_engine::HC_PREFIX + 2 * k - e->hc_abs0);
    c16 v; v.r = (int16_t)(((int)b[0] - 127) * 64); v.i = (int16_t)(((int)b[1] - 127) * 64);
    return v;
}

// what decim[0]'s last compaction inside the first n input samples of the session leaves at the front of its window (StaleWindows, nrsc5_dev.h; the device-side
// form is hb_roll_history, k_decimate.hip): false = no compaction in that span, `out` untouched
bool nrsc5::hc_stale_hb(const nrsc5hip_engine *e, long long n, c16 out[14])
{
    const long long p = stale_start(0, n, 14);
    if (p == STALE_NONE) return false;
    for (int k = 0; k < 14; k++) out[k] = hc_sample_q15(e, p + k);
    return true;
}

// a freshly reset FM stream's first cu8 push: bind the buffer to it if its decimator history is expressible as input bytes (always, unless an AM session's
// >> 4 samples were left in decim[0]'s window)
static int hc_try_attach(nrsc5hip_engine *e, int s)
{
    uint8_t pre[nrsc5hip_engine::HC_PREFIX];
    memset(pre, 0x7f, sizeof(pre));
    for (int k = 0; k < 14; k++) {
        const c16 h = e->hb_hist_host[s][k];
        if ((h.r & 63) || (h.i & 63)) return 0;
        const int r = h.r / 64 + 127, i = h.i / 64 + 127;
        if (r < 0 || r > 255 || i < 0 || i > 255) return 0;
        pre[nrsc5hip_engine::HC_PREFIX - 28 + 2 * k] = (uint8_t)r; pre[nrsc5hip_engine::HC_PREFIX - 28 + 2 * k + 1] = (uint8_t)i;
    }
    int rc = settle(e); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->main));
    memcpy(e->hc_pin, pre, sizeof(pre));
    e->hc_abs0 = 0; e->hc_wr = nrsc5hip_engine::HC_PREFIX;
    // wr, rd, base, raw are the first four members of StreamState: the stream reads the capture from dword HC_OFF on, and the HOST decides when a window is complete
    // (the fast seam steps a stream only when its mirror says so), so the device-side end of data is set out of reach
    struct { long long wr, rd, base; const uint8_t *raw; } head = { 1ll << 60, nrsc5hip_engine::HC_OFF, 0, e->hc_dev };
    static_assert(offsetof(StreamState, wr) == 0 && offsetof(StreamState, rd) == 8 && offsetof(StreamState, base) == 16 && offsetof(StreamState, raw) == 24, "StreamState head layout");
    HIPCHK(hipMemcpy(e->db.state + s, &head, sizeof(head), hipMemcpyHostToDevice));
    e->wr_host[s] = e->rd_host[s] = nrsc5hip_engine::HC_OFF; e->base_host[s] = 0;
    e->hc_stream = s; e->hc_attaches++;
    return 0;
}

// the buffer is full: the live tail -- HC_KEEP bytes behind the read position (the decimator taps, and what a reset needs to tell the stale window) up to the write
// position -- moves to the front, and the stream's `raw` with it.  Nothing may be reading: every step is harvested first.
static int hc_rebase(nrsc5hip_engine *e)
{
    const int s = e->hc_stream;
    int rc = settle(e); if (rc) return rc;
    long long from = (4 * e->rd_host[s] - nrsc5hip_engine::HC_KEEP) & ~63ll;
    if (from <= e->hc_abs0) FAIL(NRSC5HIP_EOVERFLOW, "stream %d: the pinned capture (%zu bytes) cannot hold one window", s, e->hc_cap);
    memmove(e->hc_pin, e->hc_pin + (from - e->hc_abs0), (size_t)(e->hc_wr - from));
    e->hc_abs0 = from;
    const uint8_t *raw = e->hc_dev - from;                     // dword d of the stream's numbering lives at raw + 4 d
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy((char *)(e->db.state + s) + offsetof(StreamState, raw), &raw, sizeof(raw), hipMemcpyHostToDevice));
    e->hc_rebases++;
    return 0;
}

// Turn the bound stream back into a FIFO stream: the device forgets the capture at its read position -- FIFO empty there, decimator history = the 14 input samples in
// front of it, decim[0]'s stale-window bookkeeping as the streaming decimator would have left it -- and the bytes behind that position go through the ordinary
// seam again (pinned staging, decimator).  For callers that leave what the capture can express: a cs16 push into the session, the batch entry points.
int nrsc5::hc_detach(nrsc5hip_engine *e)
{
    const int s = e->hc_stream;
    if (s < 0) return 0;
    int rc = settle(e); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->main));
    const long long rd = e->rd_host[s], consumed = 2 * (rd - nrsc5hip_engine::HC_OFF);   // input samples in front of the read position
    struct { long long wr, rd, base; const uint8_t *raw; c16 hb_hist[14]; } head = { rd, rd, rd, nullptr, {} };
    static_assert(offsetof(StreamState, hb_hist) == 32, "StreamState head layout");
    for (int k = 0; k < 14; k++) head.hb_hist[k] = hc_sample_q15(e, consumed - 14 + k);
    HIPCHK(hipMemcpy(e->db.state + s, &head, sizeof(head), hipMemcpyHostToDevice));
    c16 sw[14];
    if (hc_stale_hb(e, consumed, sw)) HIPCHK(hipMemcpy((char *)(e->db.state + s) + offsetof(StreamState, stale) + offsetof(StaleWindows, hb), sw, sizeof(sw), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((char *)(e->db.state + s) + offsetof(StreamState, stale) + offsetof(StaleWindows, hb_pushed), &consumed, sizeof(consumed), hipMemcpyHostToDevice));
    e->wr_host[s] = rd; e->base_host[s] = rd;
    e->hc_stream = -1; e->hc_detaches++;
    const long long tail0 = 4 * rd, ntail = e->hc_wr - tail0;
    if (ntail > 0) {
        // (the source is the pinned capture itself: nothing writes it while the stream is unbound)
        const bool keep = e->host_capture; e->host_capture = false;
        const char manual = e->manual_step[s]; e->manual_step[s] = 1;      // the re-push only restores the FIFO: it completes at most the window the caller has not stepped yet
        rc = push_common(e, s, e->hc_pin + (tail0 - e->hc_abs0), (size_t)ntail, true);
        e->manual_step[s] = manual; e->host_capture = keep;
        if (rc) return rc;
    }
    return 0;
}

static int push_common(nrsc5hip_engine *e, int s, const void *host, size_t nbytes_total, bool cu8)
{
    int rc = check_stream(e, s); if (rc) return rc;
    const uint8_t *src = (const uint8_t *)host;
    const size_t unit = 4;                                     // cu8: 2 complex samples; cs16: 1 complex sample
    if (nbytes_total % unit) FAIL(NRSC5HIP_EINVAL, "length must be a multiple of %zu bytes", unit);
    const bool am = e->mode_host[s] == MODE_AM;
    if (e->attached[s]) FAIL(NRSC5HIP_EINVAL, "stream %d reads a zero-copy capture: reset it before pushing samples", s);
    const bool fast = !e->cfg.p1_async && e->mirror_ok[s];
    if (e->ahead.valid && (rc = harvest(e, true))) return rc;  // the mirror lacks a step submitted ahead until its predecessor is harvested
    while (e->inflight_stream >= 0 && (!fast || e->inflight_stream != s)) if ((rc = harvest(e, true))) return rc;
    if (e->hc_stream == s && (!fast || !cu8 || am) && (rc = hc_detach(e))) return rc;      // the capture holds FM cu8 input of the fast seam, nothing else
    if (fast && cu8 && !am && e->host_capture && e->hc_stream < 0 && e->wr_host[s] == 0 && e->rd_host[s] == 0 && e->staged_stream != s && nbytes_total &&
        (rc = hc_try_attach(e, s))) return rc;
    const bool hc = e->hc_stream == s;
    if (fast && e->staged_stream >= 0 && (e->staged_stream != s || e->staged_cu8 != cu8) && (rc = flush_staged(e))) return rc;
    if (fast && e->manual_step[s] && e->wr_host[s] - e->rd_host[s] >= window_of(e, s) && (rc = stream_steps(e, s))) return rc;   // the caller did not step
    while (nbytes_total) {
        if (hc) {
            // host-resident capture: the bytes stay where this copy puts them; a block is stepped when the mirror says its window is complete
            size_t chunk = nbytes_total;
            const long long to_block = nrsc5hip_bytes_to_next_block(e, s, 1);      // (as below: block by block, whatever the size of the push)
            if (to_block > 0 && (size_t)to_block < chunk) chunk = (size_t)to_block;
            if ((size_t)(e->hc_wr - e->hc_abs0) + chunk > e->hc_cap && (rc = hc_rebase(e))) return rc;
            if ((size_t)(e->hc_wr - e->hc_abs0) + chunk > e->hc_cap) FAIL(NRSC5HIP_EOVERFLOW, "stream %d: the pinned capture (%zu bytes) is too small", s, e->hc_cap);
            { SeamClock clk(0); memcpy(e->hc_pin + (e->hc_wr - e->hc_abs0), src, chunk); }
            g_seam[4] += 1; g_seam[13] += 1;
            e->hc_wr += (long long)chunk; e->wr_host[s] += (long long)chunk / 4;
            src += chunk; nbytes_total -= chunk;
            if (e->wr_host[s] - e->rd_host[s] >= window_of(e, s)) {
                if (e->manual_step[s] && nbytes_total == 0) break;     // nrsc5hip_stream_step runs the block
                if ((rc = stream_steps(e, s))) return rc;
            }
            continue;
        }
        if (fast) {
            // stage in pinned memory; submit when the block completes (the mirror knows) or the buffer is full
            const int slot = e->stage_slot;
            if (e->staged_bytes == 0 && e->stage_busy[slot]) { SeamClock clk(1); HIPCHK(hipEventSynchronize(e->stage_ev[slot])); e->stage_busy[slot] = false; }
            const size_t room = e->stage_ring_bytes - e->staged_bytes;
            size_t chunk = nbytes_total > room ? room : nbytes_total;
            // never stage past the sample that completes the stream's next block: a large push is then processed block by block and
            // the FIFO never holds more than one window plus the carry of the last block, whatever q15_capacity is (>= 2 windows)
            const long long to_block = nrsc5hip_bytes_to_next_block(e, s, cu8 ? 1 : 0);
            if (to_block > 0 && (size_t)to_block < chunk) chunk = (size_t)to_block;
            long long nq15 = (long long)chunk / 4;
            if (am && cu8) nq15 = (e->raw_host[s] + (long long)chunk / 2) / 32 - e->raw_host[s] / 32;
            { SeamClock clk(0); memcpy(e->stage_pin[slot] + 16 + e->staged_bytes, src, chunk); }
            g_seam[4] += 1;
            e->staged_stream = s; e->staged_cu8 = cu8; e->staged_bytes += chunk; e->staged_q15 += nq15;
            e->wr_host[s] += nq15;
            if (am && cu8) e->raw_host[s] += (long long)chunk / 2;
            src += chunk; nbytes_total -= chunk;
            if (e->wr_host[s] - e->rd_host[s] >= window_of(e, s) || e->staged_bytes == e->stage_ring_bytes) {
                if ((rc = flush_staged(e))) return rc;
                if (e->manual_step[s] && nbytes_total == 0) break;     // samples are on their way to the FIFO; nrsc5hip_stream_step runs the block
                if ((rc = stream_steps(e, s))) return rc;
            } else if (e->early_flush && e->staged_bytes >= e->early_flush && cu8 && !am && e->direct_decimate) {
                if ((rc = flush_staged(e))) return rc;         // ahead of the block's end, beside the step that is running
            }
            continue;
        }
        const size_t chunk = nbytes_total > e->stage_bytes ? e->stage_bytes : nbytes_total;
        long long nq15 = (long long)chunk / 4;                  // FM cu8: 2:1; cs16: one complex sample per 4 bytes
        if (am && cu8) nq15 = (e->raw_host[s] + (long long)chunk / 2) / 32 - e->raw_host[s] / 32;
        if ((rc = ensure_space(e, s, nq15))) return rc;
        const unsigned count = cu8 ? (unsigned)chunk : (unsigned)(chunk / 2);
        e->mirror_ok[s] = 0; e->pending[s].clear(); e->fetched[s] = e->drained[s]; forget_prediction(e, s); e->counters_clean = false;
        HIPCHK(hipMemcpyAsync(e->stage_dev, src, chunk, hipMemcpyHostToDevice, e->main));
        HIPCHK(hipMemcpyAsync(e->ids_dev, &s, sizeof(int), hipMemcpyHostToDevice, e->main));
        HIPCHK(hipMemcpyAsync(e->nbytes_dev, &count, sizeof(unsigned), hipMemcpyHostToDevice, e->main));
        HIPCHK(hipStreamSynchronize(e->main));                 // &s / &count are stack temporaries
        if (cu8 && am) { launch_am_decimate_cu8(e->tb, e->db, 1, e->ids_dev, e->stage_dev, 0, e->nbytes_dev, count, e->main); e->raw_host[s] += (long long)chunk / 2; }
        else if (cu8) launch_decimate_fm_cu8(e->tb, e->db, 1, e->ids_dev, e->stage_dev, 0, e->nbytes_dev, count, e->main);
        else launch_append_cs16(e->db, 1, e->ids_dev, (const int16_t *)e->stage_dev, 0, e->nbytes_dev, count, e->main);
        e->wr_host[s] += nq15;
        int steps = 0;
        if (am) { if ((rc = run_steps_am(e, 1, e->ids_dev, 1 << 30, 1, &steps))) return rc; }
        else if ((rc = run_steps(e, 1, e->ids_dev, set_signature(1, &s), 1 << 30, 1, &steps))) return rc;
        src += chunk; nbytes_total -= chunk;
    }
    return 0;
}

extern "C" int nrsc5hip_push_cu8(nrsc5hip_engine *e, int stream, const uint8_t *iq, uint32_t nbytes)
{
    ON_ENGINE_DEVICE_FAST(e);
    return push_common(e, stream, iq, nbytes, true);
}
extern "C" int nrsc5hip_push_cs16(nrsc5hip_engine *e, int stream, const int16_t *iq, uint32_t n)
{
    ON_ENGINE_DEVICE_FAST(e);
    if (n % 2) FAIL(NRSC5HIP_EINVAL, "cs16 length must be even");
    return push_common(e, stream, iq, (size_t)n * 2, false);
}

// ---- results ------------------------------------------------------------------------------------------------------
static int fetch_nblocks(nrsc5hip_engine *e, int s, int *nblocks)
{
    HIPCHK(hipMemcpy(nblocks, (const char *)(e->db.state + s) + offsetof(StreamState, nblocks), sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nrsc5hip_drain(nrsc5hip_engine *e, int stream, nrsc5hip_record *out, int max, int *n_out)
{
    ON_ENGINE_DEVICE_FAST(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (!out || !n_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    // the block step in flight is waited for; samples that are still being decimated on the ingest stream are not (a drop-in session
    // drains right after it has submitted the last chunk of the next block: waiting for that kernel was ~20 us per block)
    if (e->inflight_stream >= 0 && (rc = harvest(e, true))) return rc;
    if (!e->mirror_ok[stream] && (rc = settle(e))) return rc;
    if (e->mirror_ok[stream]) {
        // fast streaming seam: every record of a finished block step is on the host already (k_stream_report)
        std::deque<BlockRecord> &q = e->pending[stream];
        int n = 0;
        for (; n < max && !q.empty(); n++) { memcpy(&out[n], &q.front(), sizeof(BlockRecord)); q.pop_front(); }
        e->drained[stream] += n;
        *n_out = n;
        return 0;
    }
    HIPCHK(hipStreamSynchronize(e->main));
    int nb = 0;
    if ((rc = fetch_nblocks(e, stream, &nb))) return rc;
    if (nb - e->drained[stream] > e->db.rec_cap) FAIL(NRSC5HIP_EOVERFLOW, "stream %d: %d records overwrote the ring (capacity %d)", stream, nb - e->drained[stream], e->db.rec_cap);
    const bool replay = e->db.ckpt || e->db.am_ckpt;
    int n = 0;
    // Replay: blocks that ran behind a failed P1 frame are void (k_replay.hip) and never delivered.  A rewind can void up to
    // NWIN * 16 records in a row, so keep reading until `max` valid records are collected or the ring is empty -- a caller that
    // loops "until fewer than max came back" must not stop at a chunk of void records.
    while (n < max && e->drained[stream] < nb) {
        const int want = std::min(max - n, nb - e->drained[stream]);
        const int first = e->drained[stream] % e->db.rec_cap;      // at most two contiguous pieces of the ring
        const int n1 = (first + want <= e->db.rec_cap) ? want : e->db.rec_cap - first;
        const BlockRecord *ring = e->db.records + (size_t)stream * e->db.rec_cap;
        HIPCHK(hipMemcpy(out + n, ring + first, (size_t)n1 * sizeof(BlockRecord), hipMemcpyDeviceToHost));
        if (want - n1 > 0) HIPCHK(hipMemcpy(out + n + n1, ring, (size_t)(want - n1) * sizeof(BlockRecord), hipMemcpyDeviceToHost));
        e->drained[stream] += want;
        int m = n;
        for (int k = n; k < n + want; k++) if (!replay || !(out[k].flags & NRSC5HIP_REC_DISCARDED)) { if (m != k) out[m] = out[k]; m++; }
        n = m;
    }
    *n_out = n;
    if (e->cfg.p1_async && e->db.am && e->mode_host[stream] == MODE_AM && n > 0) return patch_am_ber(e, stream, out, n, nullptr);
    return 0;
}

// The drop-in's form of drain: whatever has been reported so far, without waiting for a block step that is still running
extern "C" int nrsc5hip_drain_ready(nrsc5hip_engine *e, int stream, nrsc5hip_record *out, int max, int *n_out)
{
    ON_ENGINE_DEVICE_FAST(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (!out || !n_out) FAIL(NRSC5HIP_EINVAL, "null argument");
    if (!e->mirror_ok[stream]) return nrsc5hip_drain(e, stream, out, max, n_out);
    if (e->inflight_stream >= 0 && (rc = harvest(e, false))) return rc;
    std::deque<BlockRecord> &q = e->pending[stream];
    int n = 0;
    for (; n < max && !q.empty(); n++) { memcpy(&out[n], &q.front(), sizeof(BlockRecord)); q.pop_front(); }
    e->drained[stream] += n;
    *n_out = n;
    return 0;
}

extern "C" int nrsc5hip_stream_set_manual_step(nrsc5hip_engine *e, int stream, int on)
{
    ON_ENGINE_DEVICE(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    e->manual_step[stream] = on ? 1 : 0;
    return 0;
}

// manual-step streams: run the block(s) whose window the pushes so far completed (the step may stay in flight: drain waits for it,
// drain_ready does not)
extern "C" int nrsc5hip_stream_step(nrsc5hip_engine *e, int stream)
{
    ON_ENGINE_DEVICE_FAST(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (e->cfg.p1_async || !e->mirror_ok[stream]) FAIL(NRSC5HIP_EINVAL, "stream %d is not driven by the fast streaming seam", stream);
    if (e->inflight_stream >= 0 && e->inflight_stream != stream && (rc = harvest(e, true))) return rc;
    if (e->staged_stream == stream && (rc = flush_staged(e))) return rc;
    return stream_steps(e, stream);
}

// manual-step streams: submit the block the pushes so far completed BEHIND the step still in flight, if that is safe; *submitted
// tells.  0: the caller drains, feeds L2 and calls nrsc5hip_stream_step as usual.
extern "C" int nrsc5hip_stream_step_ahead(nrsc5hip_engine *e, int stream, int *submitted)
{
    ON_ENGINE_DEVICE_FAST(e);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (!submitted) FAIL(NRSC5HIP_EINVAL, "null argument");
    *submitted = 0;
    if (e->cfg.p1_async || !e->mirror_ok[stream] || !e->manual_step[stream] || !e->defer_wait || e->cfg.l2_feedback || e->prof_on) return 0;
    if (e->mode_host[stream] == MODE_AM || e->ahead.valid) return 0;
    // the step in flight: same stream, started FINE (predicted), no P1 decode -> its delivery cannot send the stream back to NONE
    if (e->inflight_stream != stream || e->inflight_rd_pred < 0 || e->inflight_decoded || !e->pred_ok[stream]) return 0;
    if (e->staged_stream == stream && (rc = flush_staged(e))) return rc;
    if (e->wr_host[stream] - e->rd_host[stream] < window_of(e, stream)) return 0;
    if ((rc = submit_step(e, stream, true))) return rc;
    *submitted = 1;
    return 0;
}

extern "C" int nrsc5hip_p1_frame_packed(nrsc5hip_engine *e, int stream, int slot, uint32_t *words)
{
    ON_ENGINE_DEVICE_FAST(e);
    SeamClock clk(7);
    int rc = check_stream(e, stream); if (rc) return rc;
    if (slot < 0 || slot >= e->db.p1_slots || !words) FAIL(NRSC5HIP_EINVAL, "bad slot/argument");
    if (e->inflight_stream >= 0 && (rc = harvest(e, true))) return rc;
    if (e->mirror_ok[stream] && e->db.p1_mirror && e->frames_host && e->mode_host[stream] != MODE_AM) {
        // fast seam (FM): the step that decoded the frame has been harvested, and its traceback wrote the frame into the pinned
        // mirror before the report kernel that the harvest waited for
        memcpy(words, e->frames_host + ((size_t)stream * e->db.p1_slots + slot) * P1_WORDS, P1_WORDS * sizeof(uint32_t));
        return 0;
    }
    if ((rc = settle(e))) return rc;
    HIPCHK(hipStreamSynchronize(e->main));
    HIPCHK(hipMemcpy(words, e->db.p1_ring + ((size_t)stream * e->db.p1_slots + slot) * P1_WORDS, P1_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}
