// What the host-side units of the engine share: the engine object, the entry-point guards, the launch profiler and the few
// helpers that cross units (engine.hip, engine_steps.hip, engine_seam.hip, engine_batch.hip, engine_stage.hip).
#pragma once
#include <string.h>
#include <array>
#include <deque>
#include <vector>
#include "kernels.h"
#include "host_util.h"

struct nrsc5hip_engine;
namespace nrsc5 {
// Helpers with external linkage live here, as the launchers do: no unmangled symbol leaves the library but the C ABI.
int settle(nrsc5hip_engine *e);                                // engine_seam.hip: nothing of the fast seam in flight
int flush_staged(nrsc5hip_engine *e);
int hc_detach(nrsc5hip_engine *e);
bool hc_stale_hb(const nrsc5hip_engine *e, long long n, c16 out[14]);
extern __thread double g_seam[14];                             // the seam's wall-clock totals (nrsc5hip_debug_seam_totals); __thread: plain TLS, no init wrapper
int leave_mirror(nrsc5hip_engine *e, int n, const int *ids);   // engine_batch.hip
int upload_ids(nrsc5hip_engine *e, int n, const int *ids, const uint32_t *counts, const int **ids_dev);
int patch_am_ber(nrsc5hip_engine *e, int stream, nrsc5hip_record *recs, int n, const float *ber_row);
int l2_run(nrsc5hip_engine *e, const std::vector<L2Job> &jobs, nrsc5hip_l2_frame *out, uint8_t *pdu_bytes, long long stride);
int l2_launch(nrsc5hip_engine *e, const std::vector<L2Job> &jobs, L2Job *djobs, nrsc5hip_l2_frame *dframes, uint8_t *dbytes, long long stride);   // device half of l2_run
int l2_resolve(nrsc5hip_engine *e, int njobs, const nrsc5hip_l2_job *jobs, std::vector<L2Job> &dj);
int run_steps(nrsc5hip_engine *e, int n, const int *ids_dev, unsigned long long set_sig, int max_steps, int check_every, int *steps_done);   // engine_steps.hip
int run_steps_am(nrsc5hip_engine *e, int n, const int *ids_dev, int max_steps, int check_every, int *steps_done);
void prof_collect(nrsc5hip_engine *e);                         // engine.hip
}
using namespace nrsc5;                                         // (a header of the engine's own units only)

// Every entry point runs on ITS ENGINE's device, whatever the calling thread's current device is (one process may own one engine
// per GPU, each driven by its own thread or all by one): the guard switches on entry and restores on exit.
#define ON_ENGINE_DEVICE_FAST(e) nrsc5::DeviceGuard _device_guard((e) ? (e)->cfg.device : 0); if (!(e)) FAIL(NRSC5HIP_EINVAL, "null engine")
// ... and, for every entry but the fast streaming seam's own, with no block step in flight (deferred wait, see nrsc5hip_engine)
#define ON_ENGINE_DEVICE(e) ON_ENGINE_DEVICE_FAST(e); do { int _rc = nrsc5::settle(e); if (_rc) return _rc; } while (0)

struct nrsc5hip_engine {
    nrsc5hip_config cfg;
    DevTables tb;
    DevBuffers db;                     // THE buffer table: every launch takes it from here
    // The block-step chain: its HIP stream, the decode streams of the window pipeline and their bookkeeping.
    hipStream_t main, aux[NAUX];
    hipEvent_t ev_window[NWIN], ev_decoded[NWIN];
    bool decoded_pending[NWIN];
    int lane_parity[NAUX];             // window slot of the last decode each decode stream was given (-1: none yet)
    bool thin;                         // the last burst advanced fewer than a quarter of the set's streams (the replaying stragglers' tail)
    bool acq_needed;                   // some stream of the CURRENT stream set may be un-synchronised: launch the acquisition kernels
    bool px_needed;                    // some stream is not FINE yet or runs a service mode with extended sidebands
    unsigned long long set_sig;        // identity of the stream set the two flags above were measured on (0 = none)
    int dec_waited;                    // chunks of the current chunked append the chain has already waited for
    bool prepared_by_sync;             // the previous step's k_sync already ran the next block's bookkeeping
    long long step_count;              // block steps issued so far (decode-window bookkeeping in async mode)
    long long am_step_count;           // same for the AM window pipeline (8 steps per window)
    bool am_decoded_pending[NWIN];
    int *counters_host;                // pinned copy of db.counters as of the last look
    int naux;                          // decode streams in use (<= NAUX)
    int naux_am;                       // ... by the AM window pipeline (2 measured best once the P3 frame decodes in segment waves)
    int verdict_lag;                   // test hook (nrsc5hip_debug_tune): replay takes verdicts this many windows late
    int am_segments, am_warm, am_runin;   // K=9 decode of the AM P3 frame: segment waves per frame (8), their forward warm-up / traceback run-in (test hooks: 0)
    int fwd_warm;                      // test hook: speculative warm-up trips of a forward segment (2; 0 makes every speculation fail -> repair path)
    int mixfft_syms;                   // symbols per k_mixfft workgroup (1, 2, 4, 8)
    int sync_lanes;                    // work-items per stream of k_sync: 0 = by the size of the stream set, 256, 768
    int fold_report;                   // 1 (default): fast seam, a step with nothing behind k_sync: k_sync posts the report (NRSC5HIP_TUNE_FOLD_REPORT = 0: k_stream_tail as a launch of its own)
    int fuse_seam_prepare;             // 1 (default): fast seam, FINE stream: no k_prepare launch (NRSC5HIP_TUNE_SEAM_PREPARE = 0: separate launch)
    int tb_walk;                       // > 0: single-path traceback (k_p1_tbwalk + check): 1 (default) = a workgroup per (frame, part), N > 1 = a persistent grid of N workgroups (opt-in); 0: the block-parallel one of round 3
    int fwd_segments;                  // waves per frame of the P1 forward pass; 0 = pick from the size of the stream set (fwd_segments_for)
    int flow_min;                      // dataflow bursts (k_flow, k_sync.hip): stream sets of at least this many streams (0 = never) run the steps of a burst in which every
                                       // stream is FINE as ONE launch
    unsigned *flow_dev; size_t flow_cap;   // its hand-off words (zeroed before every launch) and how many there are
    unsigned *flow_err;                    // two words of pinned host memory the kernel writes when a poll gives up
    long long flow_bursts, flow_steps;     // bursts / block steps issued that way since the engine was created
    std::vector<void *> allocs;
    // host mirrors
    std::vector<long long> wr_host, base_host;
    std::vector<int> drained;          // records already handed out per stream
    std::vector<int> mode_host;        // MODE_FM / MODE_AM per stream
    std::vector<long long> raw_host;   // AM cu8: raw input samples consumed (32:1 decimator phase)
    std::vector<char> attached;        // zero-copy batch: the stream reads the caller's capture (one append per reset)
    // Fast streaming seam (p1_async = 0): the host mirrors the stream's FIFO read position, so a push that cannot complete a
    // block costs one host memcpy into pinned memory, one async H2D and the K1 launch -- no synchronisation at all -- and a
    // push that does complete one ends with ONE sync, after a report kernel has posted the counters, the new read position and
    // the block's record straight into pinned host memory.
    // NSTAGE pinned staging buffers used round robin (a buffer is refilled NSTAGE submissions after it was handed to the device: with
    // two, and three submissions per block, the host waited ~30 us per block for the decimator of the submission before last)
    static constexpr int NSTAGE = 8;
    uint8_t *stage_pin[NSTAGE], *stage_pin_dev[NSTAGE], *stage_dev2[NSTAGE]; hipEvent_t stage_ev[NSTAGE]; bool stage_busy[NSTAGE]; int stage_slot;
    unsigned *decim_ticket;            // k_decimate_fm_cu8_stream: workgroups of the running launch that have finished
    // Ingest stream (round 4): the direct decimator runs on its own HIP stream, beside the block step on `main` (which keeps ONE CU
    // busy): chunks are submitted as they fill (early_flush bytes), so that when the push that completes a block arrives only the
    // remainder is left to decimate and nothing of it sits on the step chain.  Order between the two streams: a step waits for the
    // ingest work submitted before it (ev_ingest); a FIFO compaction on the ingest stream waits for the steps submitted before it
    // (ev_main: it needs the final read position); anything else that touches the stream synchronises both (settle).
    hipStream_t ingest; hipEvent_t ev_ingest, ev_main, ev_appended;
    bool ingest_dirty;                 // work on the ingest stream that `main` has not been ordered behind yet
    bool main_stepped;                 // block steps on `main` that the ingest stream has not been ordered behind yet
    bool main_appended;                // FIFO appends on `main` (a block's last chunk) that the ingest stream has not been ordered behind yet
    size_t early_flush;                // staged bytes at which a chunk is submitted before its block is complete (0: never)
    // samples accepted by a push but not submitted yet: they wait in stage_pin[stage_slot] until the mirror says a block completes
    // (or the buffer is full, or anything else looks at the stream) -- one H2D + one decimator launch per BLOCK, not per push
    int staged_stream; size_t staged_bytes; bool staged_cu8; long long staged_q15;
    StreamReport *report_host[2], *report_dev[2];   // pinned, device-mapped reports: the step with sequence number q posts into [q & 1]
    std::vector<long long> rd_host;            // FIFO read position (absolute decimated samples) as of the last report
    std::vector<int> fetched;                  // records of the stream copied to `pending` so far (absolute index)
    std::vector<char> mirror_ok;               // rd_host / pending are exact: only the streaming seam touched the stream since its reset
    std::vector<std::deque<BlockRecord>> pending;   // records reported but not yet drained
    // Deferred wait (round 4).  A block that starts in FINE consumes a number of samples the host can compute in advance
    // (keep = 2160 - the timing feedback of the previous block, acquire.c:112,259; both are in that block's record), so the mirror
    // is advanced at SUBMISSION and the wait for the step's report moves to the next call that needs its results: the device works
    // on block n while the host copies the pushes of block n + 1 into staging.  At most one step per engine is in flight.
    int inflight_stream;               // stream whose block step is submitted but not harvested (-1: none)
    unsigned report_seq;               // sequence number the most recently launched report kernel posts when it is done
    long long inflight_rd_pred;        // the read position predicted for the step in flight (-1: no prediction, the mirror waits)
    bool inflight_decoded;             // the step in flight carried the P1 de-interleave / trellis / traceback launches
    unsigned inflight_seq;             // its report's sequence number
    // A second step, submitted AHEAD of the delivery of the one in flight (nrsc5hip_stream_step_ahead): allowed when the block in
    // flight starts FINE and cannot complete a P1 frame -- nothing its delivery tells the host can change what the next block does
    // (frame.c's only way back into L1 is the first header of a P1 frame, frame.c:535-540) -- so the device runs block n + 1 while
    // the host still hands block n to L2.  Its read-position prediction needs block n's record: it is made when that is harvested.
    struct Ahead { bool valid; int stream; unsigned seq; bool decoded; } ahead;
    bool inflight_progress;            // the last harvested step processed (or left pending) a block
    bool direct_decimate;              // 1 (default): FM cu8 pushes are decimated straight from the pinned staging buffer; 0 (NRSC5HIP_TUNE_DIRECT_DECIMATE): H2D copy first
    bool defer_wait;                   // 1 (default): predictable steps stay in flight; 0 (NRSC5HIP_TUNE_DEFER_WAIT): every step is waited for at once
    bool counters_clean;               // the step counters are zero: the last kernel that touched them was a report kernel
    std::vector<char> pred_ok;         // the stream's last harvested record left it FINE and nothing else touched it since
    std::vector<int> pred_samperr, pred_bc;    // ... that record's next_samperr and block count
    std::vector<char> manual_step;     // nrsc5hip_stream_set_manual_step: pushes stage and submit samples, the caller steps
    // Host-resident capture (round 6; fast seam, FM cu8, NRSC5HIP_TUNE_HOST_CAPTURE): the pushes of ONE stream of the engine are kept as they arrive in a pinned,
    // device-mapped buffer and the stream reads them in place -- StreamState::raw points into it, and the symbol kernel / the acquisition run the half-band on what they
    // read (halfband_raw.h): the zero-copy batch's kernels, fed across PCIe.  A push is one host memcpy: no decimator launch, no ingest stream, nothing in front of the
    // block step.  The stream's own byte numbering: HC_PREFIX bytes of decimator history (what its reset left in hb_hist), then every byte pushed since that reset;
    // decimated sample a = dword a of that numbering, so the stream's counters start at HC_OFF.  The buffer is linear: when it is full the live tail moves to its
    // front and `raw` moves with it (hc_rebase).  Anything the capture cannot express (a cs16 push, the batch entry points) first turns it back into the FIFO (hc_detach).
    static constexpr long long HC_OFF = 8, HC_PREFIX = 4 * HC_OFF, HC_KEEP = 16384;
    uint8_t *hc_pin, *hc_dev; size_t hc_cap;
    int hc_stream;                     // the stream bound to the buffer, -1: none
    long long hc_abs0, hc_wr;          // byte index (stream numbering) of hc_pin[0] / of the next byte to be written
    bool host_capture;                 // knob (default on where the buffer exists)
    long long hc_rebases, hc_attaches, hc_detaches;
    long long reports_folded;          // block steps whose report the sync kernel posted itself (fold_report)
    std::vector<std::array<c16, 14>> hb_hist_host;   // the decimator history each stream's last reset left on the device (zeros for a fresh session)
    // staging
    uint8_t *stage_dev; size_t stage_bytes;
    size_t stage_ring_bytes;           // size of each of the NSTAGE staging buffers of the fast seam (a block of either mode fits)
    int *ids_dev; unsigned *nbytes_dev;
    int *all_ids_dev;                  // identity list 0..S-1
    TrimPlan *trim_plan_dev;           // nrsc5hip_batch_trim: one plan per listed stream (k_trim.hip)
    // chunked K1 running ahead of the block steps on its own stream (fresh batches in the async pipeline)
    hipStream_t dec_stream;
    std::vector<hipEvent_t> dec_events;    // dec_events[c] fires when output samples [0, (c+1)*dec_chunk) of every stream are committed
    long long dec_chunk;                   // output samples per chunk, 0 = no chunked append outstanding
    unsigned *chunk_nbytes_dev; int chunk_cap;
    // engine-owned pinned result buffers for nrsc5hip_batch_fetch_view (allocated on first use)
    BlockRecord *rec_host; uint32_t *frames_host; int *nblocks_host;
    // optional per-kernel-class timing with HIP events on the launching stream
    bool prof_on;
    int prof_only;                     // -1: every class is timed; else only this one (events cost ~5 us of the chain's time per kernel)
    struct ProfSpan { int cls; hipEvent_t a, b; };
    std::vector<ProfSpan> prof_spans;
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[NRSC5HIP_PROF_CLASSES];
    long long prof_launches[NRSC5HIP_PROF_CLASSES];
    long long *sync_phase_buf;         // k_sync's phase timers (NRSC5HIP_TUNE_SYNC_PHASES): allocated on first use; db.sync_phase_cycles points here while they are on
    VitScratch vit_scratch;            // scratch of the nrsc5hip_stage_viterbi_* entry points (per engine: nothing process-global)
};

static inline hipEvent_t prof_event(nrsc5hip_engine *e)
{
    if (!e->prof_pool.empty()) { hipEvent_t ev = e->prof_pool.back(); e->prof_pool.pop_back(); return ev; }
    hipEvent_t ev = nullptr; (void)hipEventCreate(&ev); return ev;
}
struct ProfScope {
    nrsc5hip_engine *e; int cls; hipStream_t st; hipEvent_t a;
    ProfScope(nrsc5hip_engine *e_, int cls_, hipStream_t st_) : e(e_), cls(cls_), st(st_), a(nullptr)
    { if (e->prof_on && (e->prof_only < 0 || e->prof_only == cls)) { a = prof_event(e); (void)hipEventRecord(a, st); } }
    ~ProfScope()
    { if (a) { hipEvent_t b = prof_event(e); (void)hipEventRecord(b, st); e->prof_spans.push_back({cls, a, b}); } }
};

template <typename T> static int dev_alloc(nrsc5hip_engine *e, T **p, size_t count)
{
    void *q = nullptr;
    hipError_t err = hipMalloc(&q, count * sizeof(T) ? count * sizeof(T) : 1);
    if (err != hipSuccess) FAIL(NRSC5HIP_ENOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(err));
    e->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}

static inline int check_stream(nrsc5hip_engine *e, int s)
{
    if (!e) FAIL(NRSC5HIP_EINVAL, "null engine");
    if (s < 0 || s >= e->cfg.max_streams) FAIL(NRSC5HIP_EINVAL, "stream %d out of range", s);
    return 0;
}
static inline int stream_at(const int *ids, int k) { return ids ? ids[k] : k; }   // entry k of a stream list; no list = the identity set
static inline void forget_prediction(nrsc5hip_engine *e, int s) { e->pred_ok[s] = 0; }

static inline unsigned long long set_signature(int n, const int *ids)
{
    unsigned long long h = 0xcbf29ce484222325ull ^ (unsigned long long)n;
    if (ids) for (int k = 0; k < n; k++) h = (h ^ (unsigned long long)(unsigned)ids[k]) * 0x100000001b3ull;
    return h | 1ull;                                           // never 0 (= "no set measured yet")
}
