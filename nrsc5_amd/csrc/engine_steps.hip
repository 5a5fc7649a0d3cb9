// The block-step scheduler: runs the steps of a stream set (block_step.h) in bursts until no stream has a complete window left --
// run_steps for FM sets, run_steps_am for AM sets -- with the decode windows, the dataflow bursts and the replay's rollbacks.
#include <algorithm>
#include "block_step.h"

// K block steps of a set whose streams are all FINE as ONE launch (k_flow, k_sync.hip): what issue_step does for each of them -- the wait for the decoder that used
// this window's buffers, the symbol and sync kernels with the next block's bookkeeping fused, the window decode behind step 15 -- with the K x 2 launches replaced
// by one grid whose workgroups hand over to each other.  The caller has checked the conditions (run_steps).
static int issue_flow_burst(nrsc5hip_engine *e, int n, const int *ids_dev, int K)
{
    const long long window = e->step_count / 16;
    const int parity = (int)(window % NWIN), slot0 = (int)(e->step_count % 16);
    if (slot0 + K > 16) FAIL(NRSC5HIP_EINVAL, "a dataflow burst does not cross a window boundary");
    if (slot0 == 0 && e->decoded_pending[parity]) {
        HIPCHK(hipStreamWaitEvent(e->main, e->ev_decoded[parity], 0));
        e->decoded_pending[parity] = false;
    }
    HIPCHK(hipMemsetAsync(e->flow_dev, 0, flow_words(n) * sizeof(unsigned), e->main));
    { ProfScope p(e, NRSC5HIP_PROF_FLOW, e->main); launch_flow(e->tb, e->db, n, ids_dev, K, e->flow_dev, e->flow_err, parity, slot0, (int)window, e->main); }
    // a poll that gave up (flow words [8], [9]): the host reads them with the burst's counters (run_steps)
    e->step_count += K;
    e->flow_bursts++; e->flow_steps += K;
    if ((e->step_count % 16) == 0) { int rc = launch_window_decode(e, n, ids_dev, parity, pick_decode_lane(e, window)); if (rc) return rc; }
    HIPCHK(hipGetLastError());
    return 0;
}

// finish a partially filled decode window (async mode) so that every produced frame gets decoded, and wait for all decodes
static int flush_p1(nrsc5hip_engine *e, int n, const int *ids_dev)
{
    if (!e->cfg.p1_async) return 0;
    if (e->step_count % 16) {
        const long long window = e->step_count / 16;
        int rc = launch_window_decode(e, n, ids_dev, (int)(window % NWIN), pick_decode_lane(e, window)); if (rc) return rc;
        e->step_count += 16 - (e->step_count % 16);            // the next steps start a fresh window
    }
    for (int k = 0; k < NAUX; k++) HIPCHK(hipStreamSynchronize(e->aux[k]));
    for (int k = 0; k < NWIN; k++) e->decoded_pending[k] = false;
    return 0;
}

// Runs block steps for the n streams listed at ids_dev until none of them has a complete window left (or max_steps).
// `set_sig` identifies the stream set: the acquisition / PX launch flags measured on one set say nothing about another.
int nrsc5::run_steps(nrsc5hip_engine *e, int n, const int *ids_dev, unsigned long long set_sig, int max_steps, int check_every, int *steps_done)
{
    if (set_sig != e->set_sig) { e->acq_needed = true; e->px_needed = true; e->set_sig = set_sig; }
    e->prepared_by_sync = false;
    const bool replay = e->db.ckpt != nullptr;
    int done = 0;
    for (;;) {
        bool live = n > 0;
        while (live && done < max_steps) {
            HIPCHK(hipMemsetAsync(e->db.counters, 0, 4 * sizeof(int), e->main));
            // While the acquisition kernels are being launched the host looks again after 4 steps instead of a whole window: they are
            // eight thin launches per step (~38 us of a ~135 us step) for as long as the LAST look saw a stream that was not FINE,
            // and every stream of a batch is past that point a few blocks after its (re-)acquisition.
            // Bursts end on window boundaries (the rollback below is launched there).
            int every = check_every;
            if (check_every == 16) {
                const int to_boundary = 16 - (int)(e->step_count % 16);
                every = e->acq_needed ? std::min(4, to_boundary) : to_boundary;   // 2 measured: the same
            }
            int burst = 0;
            // dataflow burst (k_flow): every stream of the set was FINE at the last look, MP1 routing only, zero-copy input, closed-form oscillator, the previous
            // step's k_sync prepared this one -- the whole burst (it ends on the window boundary) is one launch
            const bool flow = e->flow_min > 0 && n >= e->flow_min && check_every == 16 && e->cfg.p1_async && e->cfg.batch_zero_copy && !e->acq_needed && !e->px_needed
                              && e->prepared_by_sync && !e->dec_chunk && e->db.nco_policy != NCO_EXACT_ALWAYS && !e->db.sync_phase_cycles && done + every <= max_steps && every >= 2;
            if (flow) { int rc = issue_flow_burst(e, n, ids_dev, every); if (rc) return rc; burst = every; }
            for (; burst < every && done + burst < max_steps; burst++) { int rc = issue_step(e, n, ids_dev); if (rc) return rc; }
            if (replay && (e->step_count % 16) == 0) {
                // Window boundary: take the first-header verdicts of the deferred decodes that have finished.  The decode whose
                // job slot the next window reuses (launched NWIN windows before it) must be among them.
                const long long window = e->step_count / 16;
                const int parity = (int)(window % NWIN);
                if (e->decoded_pending[parity]) { HIPCHK(hipStreamWaitEvent(e->main, e->ev_decoded[parity], 0)); e->decoded_pending[parity] = false; }
                ProfScope p(e, NRSC5HIP_PROF_PREPARE, e->main);
                launch_rollback(e->db, n, ids_dev, (int)window, e->verdict_lag, e->main);
            }
            HIPCHK(hipMemcpyAsync(e->counters_host, e->db.counters, 4 * sizeof(int), hipMemcpyDeviceToHost, e->main));
            HIPCHK(hipStreamSynchronize(e->main));
            if (flow && (e->flow_err[0] || e->flow_err[1]))
                FAIL(NRSC5HIP_EHIP, "dataflow burst: a hand-off was never seen (symbol item of stream position %d, block step of %d): the burst's results are void", (int)e->flow_err[0] - 1, (int)e->flow_err[1] - 1);
            e->acq_needed = e->counters_host[1] > 0;
            e->thin = e->counters_host[0] * 4 < burst * n;
            e->px_needed = e->counters_host[2] > 0;
            if (e->counters_host[0] == 0) live = false;        // nothing was processed (or is pending) in this burst
            else done += burst;
        }
        if (e->dec_chunk) { HIPCHK(hipStreamSynchronize(e->dec_stream)); e->dec_chunk = 0; }
        { int rc = flush_p1(e, n, ids_dev); if (rc) return rc; }
        if (!replay) break;
        // every decode has finished: apply what is left of their verdicts (also when the step budget is used up -- the caller
        // must never see records of blocks that ran behind a failed frame); a rewound stream has work again
        HIPCHK(hipMemsetAsync(e->db.counters, 0, 4 * sizeof(int), e->main));
        launch_rollback(e->db, n, ids_dev, (int)(e->step_count / 16), 0, e->main);
        HIPCHK(hipMemcpyAsync(e->counters_host, e->db.counters, 4 * sizeof(int), hipMemcpyDeviceToHost, e->main));
        HIPCHK(hipStreamSynchronize(e->main));
        if (e->counters_host[3] == 0) break;
        e->acq_needed = true; e->prepared_by_sync = false;
        if (done >= max_steps) break;                              // out of budget: the rewound streams resume on the next call
    }
    HIPCHK(hipStreamSynchronize(e->main));
    if (e->prof_on) prof_collect(e);
    if (steps_done) *steps_done = done;
    return 0;
}

// AM streams: one fused kernel per block step (k_am.hip).  p1_async = 0: every frame decodes in order on the main stream
// (reference event timing).  p1_async = 1: window pipeline as for FM -- each 8-step window hands the L1 frames whose
// de-interleave fell into it to one of the decode streams, where their 8 P1 frames and P3 frame decode concurrently.
static int am_flush(nrsc5hip_engine *e, int n, const int *ids_dev)
{
    if (!e->cfg.p1_async) return 0;
    if (e->am_step_count % 8) {
        const long long window = e->am_step_count / 8;
        const int parity = (int)(window % NWIN), lane = (int)(window % e->naux_am);
        hipStream_t ax = e->aux[lane];
        HIPCHK(hipEventRecord(e->ev_window[parity], e->main));
        HIPCHK(hipStreamWaitEvent(ax, e->ev_window[parity], 0));
        { ProfScope p(e, NRSC5HIP_PROF_AM_DECODE, ax); launch_am_decode(e->tb, e->db, n, ids_dev, parity, lane, e->cfg.l2_feedback, ax, e->am_segments, e->am_warm, e->am_runin); }
        e->am_step_count += 8 - (e->am_step_count % 8);
    }
    for (int k = 0; k < NAUX; k++) HIPCHK(hipStreamSynchronize(e->aux[k]));
    for (int k = 0; k < NWIN; k++) e->am_decoded_pending[k] = false;
    return 0;
}

int nrsc5::run_steps_am(nrsc5hip_engine *e, int n, const int *ids_dev, int max_steps, int check_every, int *steps_done)
{
    const bool pipe = e->cfg.p1_async != 0;
    const bool replay = e->db.am_ckpt != nullptr;              // window pipeline with the on-device L2 feedback (k_replay.hip)
    int done = 0;
    for (;;) {
        bool live = n > 0;
        while (live && done < max_steps) {
            HIPCHK(hipMemsetAsync(e->db.counters, 0, 4 * sizeof(int), e->main));
            int burst = 0;
            for (; burst < check_every && done + burst < max_steps; burst++) {
                const long long window = e->am_step_count / 8;
                const int parity = pipe ? (int)(window % NWIN) : -1, lane = (int)(window % e->naux_am);
                if (pipe && (e->am_step_count % 8) == 0) {
                    // window boundary: the decode that used this window's buffers NWIN windows ago must have finished; with the
                    // replay, take the first-header verdicts of every deferred decode that has (its job slot is reused next) --
                    // no host round trip: the burst runs on across window boundaries
                    if (e->am_decoded_pending[parity]) { HIPCHK(hipStreamWaitEvent(e->main, e->ev_decoded[parity], 0)); e->am_decoded_pending[parity] = false; }
                    if (replay && e->am_step_count > 0) launch_rollback_am(e->db, n, ids_dev, (int)window, e->verdict_lag, e->main);
                }
                { ProfScope p(e, NRSC5HIP_PROF_AM, e->main); launch_am_step(e->tb, e->db, n, ids_dev, e->main, e->cfg.l2_feedback, parity, (int)(e->am_step_count % 8), (int)window); }
                if (pipe && (e->am_step_count % 8) == 7) {
                    hipStream_t ax = e->aux[lane];
                    HIPCHK(hipEventRecord(e->ev_window[parity], e->main));
                    HIPCHK(hipStreamWaitEvent(ax, e->ev_window[parity], 0));
                    { ProfScope p(e, NRSC5HIP_PROF_AM_DECODE, ax); launch_am_decode(e->tb, e->db, n, ids_dev, parity, lane, e->cfg.l2_feedback, ax, e->am_segments, e->am_warm, e->am_runin); }
                    HIPCHK(hipEventRecord(e->ev_decoded[parity], ax));
                    e->am_decoded_pending[parity] = true;
                }
                e->am_step_count++;
            }
            HIPCHK(hipMemcpyAsync(e->counters_host, e->db.counters, 4 * sizeof(int), hipMemcpyDeviceToHost, e->main));
            HIPCHK(hipStreamSynchronize(e->main));
            HIPCHK(hipGetLastError());
            if (e->counters_host[0] == 0) live = false;
            else done += burst;
        }
        { int rc = am_flush(e, n, ids_dev); if (rc) return rc; }
        if (!replay) break;
        // every decode has finished: apply what is left of their verdicts (also when the step budget is used up); a rewound
        // stream has work again
        HIPCHK(hipMemsetAsync(e->db.counters, 0, 4 * sizeof(int), e->main));
        launch_rollback_am(e->db, n, ids_dev, (int)(e->am_step_count / 8), 0, e->main);
        HIPCHK(hipMemcpyAsync(e->counters_host, e->db.counters, 4 * sizeof(int), hipMemcpyDeviceToHost, e->main));
        HIPCHK(hipStreamSynchronize(e->main));
        if (e->counters_host[3] == 0 || done >= max_steps) break;
    }
    HIPCHK(hipStreamSynchronize(e->main));
    if (e->prof_on) prof_collect(e);
    if (steps_done) *steps_done = done;
    return 0;
}
