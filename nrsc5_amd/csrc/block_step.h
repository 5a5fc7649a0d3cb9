// ONE block step of a stream set (issue_step) and the P1 decode launches behind it.  The scheduler (engine_steps.hip) and the fast
// streaming seam (engine_seam.hip) both issue steps; the seam does it once per block of a host-paced session, inside the chain
// push_common -> flush_staged -> submit_step -> issue_step -> launch_report -> harvest that was one translation unit of static
// functions.  So the step is a header of static functions, compiled into both units: either call chain stays inlinable.
#pragma once
#include "engine_internal.h"

// One step = every listed stream whose 33-symbol window is complete advances by one block:
//   [acquisition kernels if any stream may be un-synchronised] -> prepare -> mix+FFT -> sync (+PIDS)
//   -> P1 de-interleave -> P1 Viterbi (in order, or deferred to the aux stream once per 16-step window).
// Decode stream of a window: round robin over the `naux` streams that keep the chip busy without starving the chain.  A THIN
// window (few streams advanced: the stragglers' tail of a pass) is latency- not throughput-bound -- a handful of one-wave
// trellis passes -- so when its regular stream is still busy it may take one of the spare streams instead of queueing.
static int pick_decode_lane(nrsc5hip_engine *e, long long window)
{
    const int lane = (int)(window % e->naux);
    auto busy = [&](int k) { return e->lane_parity[k] >= 0 && hipEventQuery(e->ev_decoded[e->lane_parity[k]]) == hipErrorNotReady; };
    if (e->thin && busy(lane))
        for (int k = e->naux; k < NAUX; k++) if (!busy(k)) return k;
    return lane;
}

// Waves per frame of the forward trellis pass: a window of a stream set of n streams holds ~n frames; give every frame as many
// segment waves as keeps the launch within one wave per SIMD (1024) -- up to 16.  Thin windows (the stragglers' tail) and
// small sets are latency-bound: 16.
static int fwd_segments_for(const nrsc5hip_engine *e, int n)
{
    if (e->fwd_segments > 0) return e->fwd_segments;
    if (e->thin) return 16;
    const int g = 1024 / (n > 0 ? n : 1);
    return g < 1 ? 1 : g > VIT3_GMAX ? VIT3_GMAX : g;          // a lone stream (the in-order seam, the drop-in): 64 segment waves
}

static int launch_window_decode(nrsc5hip_engine *e, int n, const int *ids_dev, int parity, int lane)
{
    // decode the window's PIDS frames and P1 frames on aux stream `lane`, overlapped with the next windows
    // (NAUX windows decode concurrently, each wave of the forward pass alone on a SIMD)
    hipStream_t ax = e->aux[lane];
    HIPCHK(hipEventRecord(e->ev_window[parity], e->main));
    HIPCHK(hipStreamWaitEvent(ax, e->ev_window[parity], 0));
    { ProfScope p(e, NRSC5HIP_PROF_PIDS, ax); launch_pids_decode(e->tb, e->db, n, ids_dev, parity, 16, ax); }
    if (e->px_needed) { ProfScope p(e, NRSC5HIP_PROF_PIDS, ax); launch_px_decode(e->tb, e->db, n, ids_dev, parity, lane, ax); }
    { ProfScope p(e, NRSC5HIP_PROF_P1_DEINT, ax); launch_p1_deint(e->tb, e->db, n, ids_dev, parity, lane, ax); }
    { ProfScope p(e, NRSC5HIP_PROF_P1_VITERBI, ax); launch_p1_forward(e->tb, e->db, n, ids_dev, parity, lane, ax, fwd_segments_for(e, n), e->fwd_warm); }
    { ProfScope p(e, NRSC5HIP_PROF_P1_TRACEBACK, ax); launch_p1_traceback(e->tb, e->db, n, ids_dev, parity, lane, ax, e->cfg.l2_feedback ? 2 : 0, fwd_segments_for(e, n), e->tb_walk); }
    HIPCHK(hipEventRecord(e->ev_decoded[parity], ax));
    e->decoded_pending[parity] = true;
    e->lane_parity[lane] = parity;
    return 0;
}

// in-order mode: the P1 frames the step's blocks completed (the kernels leave at once for a stream without one)
static int launch_inorder_p1(nrsc5hip_engine *e, int n, const int *ids_dev)
{
    { ProfScope p(e, NRSC5HIP_PROF_P1_DEINT, e->main); launch_p1_deint(e->tb, e->db, n, ids_dev, 0, 0, e->main); }
    { ProfScope p(e, NRSC5HIP_PROF_P1_VITERBI, e->main); launch_p1_forward(e->tb, e->db, n, ids_dev, 0, 0, e->main, fwd_segments_for(e, n), e->fwd_warm); }
    { ProfScope p(e, NRSC5HIP_PROF_P1_TRACEBACK, e->main); launch_p1_traceback(e->tb, e->db, n, ids_dev, 0, 0, e->main, e->cfg.l2_feedback ? 1 : 0, fwd_segments_for(e, n), e->tb_walk); }
    return 0;
}

// decode_p1 = false (fast streaming seam only): the caller KNOWS that no listed stream can complete a P1 frame in this step
// local_prepare (fast streaming seam, stream known to be FINE): no k_prepare launch -- the symbol kernel computes the block's
// bookkeeping for itself and the sync kernel commits it
struct StepReport { StreamReport *out; unsigned seq; int first_rec; bool folded; };   // fast seam: the report the step's last kernel may post itself (issue_step sets `folded` when k_sync did)
static int issue_step(nrsc5hip_engine *e, int n, const int *ids_dev, bool decode_p1 = true, bool decode_pids = true, bool local_prepare = false, StepReport *rep = nullptr)
{
    const bool async = e->cfg.p1_async != 0;
    const long long window = e->step_count / 16;
    const int parity = async ? (int)(window % NWIN) : 0;       // buffer slot of this decode window
    if (async && (e->step_count % 16) == 0 && e->decoded_pending[parity]) {
        // the buffers of slot `parity` are about to be rewritten: the decoder launched NWIN windows ago must be done
        HIPCHK(hipStreamWaitEvent(e->main, e->ev_decoded[parity], 0));
        e->decoded_pending[parity] = false;
    }
    if (e->dec_chunk) {
        // a stream starting from a fresh reset has read at most 70199 t + 71280 samples when step t begins
        const long long reach = 70199LL * e->step_count + WIN_N;
        int need = (int)(reach / e->dec_chunk) + 1;
        if (need > (int)e->dec_events.size()) need = (int)e->dec_events.size();
        for (; e->dec_waited < need; e->dec_waited++) HIPCHK(hipStreamWaitEvent(e->main, e->dec_events[e->dec_waited], 0));
    }
    if (e->cfg.l2_feedback && !async) e->acq_needed = true;   // an in-order P1 decode may send any stream back to NONE for the next block
    if (e->acq_needed) { ProfScope p(e, NRSC5HIP_PROF_ACQUIRE, e->main); launch_acquire(e->tb, e->db, n, ids_dev, e->main); }
    // prepare_block is idempotent for a stream the previous k_sync already prepared; a stream that is not FINE is only
    // prepared here, on a step that ran the acquisition kernels for its current window
    const bool fused_prepare = local_prepare && !e->acq_needed && !async && e->db.nco_policy != NCO_EXACT_ALWAYS;
    if (!fused_prepare && (!e->prepared_by_sync || e->acq_needed)) { ProfScope p(e, NRSC5HIP_PROF_PREPARE, e->main); launch_prepare(e->db, n, ids_dev, e->acq_needed ? 1 : 0, e->main); }
    // exact-oscillator blocks (a freshly reset stream up to its first lock): only a stream that is not FINE can be in that mode, and
    // those only advance on steps that run the acquisition kernels
    if (e->db.nco_tab && (e->acq_needed || e->db.nco_policy == NCO_EXACT_ALWAYS)) { ProfScope p(e, NRSC5HIP_PROF_PREPARE, e->main); launch_nco_exact(e->db, n, ids_dev, e->main); }
    { ProfScope p(e, NRSC5HIP_PROF_MIXFFT, e->main); launch_mixfft(e->tb, e->db, n, ids_dev, e->main, e->mixfft_syms, fused_prepare ? 1 : 0); }
    const int slot = async ? (int)(e->step_count % 16) : 0;
    // batch pipeline: once every stream of the set is FINE, the next block's bookkeeping rides in k_sync's tail
    const int fuse = (async && !e->acq_needed) ? 1 : 0;
    // nothing runs behind k_sync on this step (no PX kernels, no separate PIDS decode, no in-order P1 decode): it posts the step's report itself
    const bool fold = rep && n == 1 && !async && !e->px_needed && !decode_pids && !decode_p1 && e->sync_lanes != 256;     // (the wide form alone has the reporting twin: k_sync_report)
    { ProfScope p(e, NRSC5HIP_PROF_SYNC, e->main); launch_sync(e->tb, e->db, n, ids_dev, parity, slot, fuse, (int)window, e->main, e->sync_lanes, decode_pids ? 0 : 1, fused_prepare ? 1 : 0, e->px_needed ? 1 : 0,
                                                                fold ? rep->out : nullptr, fold ? rep->seq : 0u, fold ? rep->first_rec : 0); }
    if (rep) rep->folded = fold;
    e->prepared_by_sync = fuse != 0;
    if (e->px_needed) { ProfScope p(e, NRSC5HIP_PROF_PIDS, e->main); launch_px_deint(e->tb, e->db, n, ids_dev, parity, slot, e->main); }
    if (!async) {
        if (decode_pids) { ProfScope p(e, NRSC5HIP_PROF_PIDS, e->main); launch_pids_decode(e->tb, e->db, n, ids_dev, parity, 1, e->main); }
        if (e->px_needed) { ProfScope p(e, NRSC5HIP_PROF_PIDS, e->main); launch_px_decode(e->tb, e->db, n, ids_dev, parity, 0, e->main); }
        if (decode_p1) { int rc = launch_inorder_p1(e, n, ids_dev); if (rc) return rc; }
    } else if ((e->step_count % 16) == 15) {
        int rc = launch_window_decode(e, n, ids_dev, parity, pick_decode_lane(e, window)); if (rc) return rc;
    }
    e->step_count++;
    HIPCHK(hipGetLastError());
    return 0;
}
