/* libnrsc5hip -- C ABI of the MI355X (gfx950) NRSC-5 demodulate/decode engine.
 *
 * This is the drop-in boundary for the reference's IQ -> L1-frame hot path.  It replaces the
 * internal seam of theori-io/nrsc5 between L4 (src/nrsc5.c) and L2 (src/frame.c, src/pids.c):
 *
 *   down-calls replaced                      reference interface (file:line)
 *   ---------------------------------------  ----------------------------------------------
 *   nrsc5hip_push_cu8                        input_push_cu8      src/input.h:42, input.c:96-117
 *   nrsc5hip_push_cs16                       input_push_cs16     src/input.h:43, input.c:119-124
 *   nrsc5hip_stream_reset                    input_reset         src/input.h:39, input.c:126-138
 *   nrsc5hip_stream_fresh                    nrsc5_close + nrsc5_open_pipe of one slot   src/nrsc5.c
 *   nrsc5hip_force_resync                    input_set_sync_state(st, SYNC_STATE_NONE) as called
 *                                            by frame_process    src/frame.c:535-540
 *   up-calls delivered as ordered records    output_advance (acquire.c:108), nrsc5_report_sync /
 *   (nrsc5hip_drain)                         _lost_sync (input.c:177-185), nrsc5_report_mer
 *                                            (sync.c:490-501), nrsc5_report_ber (decode.c:458),
 *                                            pids_frame_push (decode.c:471, pids.h:98),
 *                                            frame_push (decode.c:460, frame.h:53)
 *
 * plus an additive batch API (device-resident captures, many independent streams per call), a wideband
 * channelizer (nrsc5hip_chan_*: one SDR capture -> one stream per station) and a band scan
 * (nrsc5hip_scan_*: the averaged power spectrum of such a capture and the centres of the hybrid-FM
 * stations in it) that the reference has no counterpart for.  All functions return 0 on success and a negative NRSC5HIP_E*
 * code on failure; nothing throws across the boundary; no C++/torch types appear in signatures.
 * Buffers passed in are borrowed for the duration of the call.  INTEGRATION.md shows the binding a
 * maintainer of the reference would add (src/input.c replacement + CMake lines).
 */
#ifndef NRSC5HIP_H_
#define NRSC5HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRSC5HIP_OK            0
#define NRSC5HIP_EINVAL       (-1)
#define NRSC5HIP_ENOMEM       (-2)
#define NRSC5HIP_EHIP         (-3)   /* a HIP runtime call failed; see nrsc5hip_last_error() */
#define NRSC5HIP_EOVERFLOW    (-4)   /* FIFO / record ring / frame ring capacity exceeded */

#define NRSC5HIP_P1_FRAME_BITS   146176   /* P1_FRAME_LEN_FM, defines.h:42 */
#define NRSC5HIP_P1_FRAME_WORDS  4568
#define NRSC5HIP_PIDS_FRAME_BITS 80       /* PIDS_FRAME_LEN, defines.h:47 */

/* waveform of a stream: NRSC5_MODE_FM / NRSC5_MODE_AM, nrsc5.h:70-74 */
enum { NRSC5HIP_MODE_FM = 0, NRSC5HIP_MODE_AM = 1 };
#define NRSC5HIP_AM_P1_FRAME_BITS  3750    /* P1_FRAME_LEN_AM, defines.h:43 */
#define NRSC5HIP_AM_P3_BITS_MA1    24000   /* P3_FRAME_LEN_MA1, defines.h:53 */
#define NRSC5HIP_AM_P3_BITS_MA3    30000   /* P3_FRAME_LEN_MA3, defines.h:54 */

/* sync states, input.h:18 */
enum { NRSC5HIP_SYNC_NONE = 0, NRSC5HIP_SYNC_COARSE = 1, NRSC5HIP_SYNC_FINE = 2 };

/* nrsc5hip_record.flags */
enum {
    NRSC5HIP_REC_PROCESSED = 1u << 0,  /* one acquire block was processed: call output_advance() first */
    NRSC5HIP_REC_TO_COARSE = 1u << 1,  /* sync state NONE -> COARSE at the top of this block */
    NRSC5HIP_REC_TO_FINE   = 1u << 2,  /* sync achieved in this block: nrsc5_report_sync(freq_offset, psmi) */
    NRSC5HIP_REC_MER       = 1u << 3,  /* nrsc5_report_mer(mer_lb, mer_ub) */
    NRSC5HIP_REC_PIDS      = 1u << 4,  /* pids_frame_push(pids) */
    NRSC5HIP_REC_P1        = 1u << 5,  /* nrsc5_report_ber(ber); frame_push(P1 frame in slot p1_slot) */
    NRSC5HIP_REC_LOST_SYNC = 1u << 6,  /* l2_feedback only: after this block's frames the engine dropped the stream to NONE (nrsc5_report_lost_sync) */
    NRSC5HIP_REC_P3        = 1u << 7,  /* FM (MP2/MP3/MP11, odd blocks): frame_push(P3 frame of PX slot `sis`, 2304 or 4608 bits);
                                          AM, block 7: frame_push(P3 frame of slot p1_slot), then nrsc5_report_ber(ber) */
    NRSC5HIP_REC_P4        = 1u << 8,  /* FM MP11: frame_push(P4 frame of PX slot `sis`, 4608 bits) */
    NRSC5HIP_REC_PIDS_CRC  = 1u << 9,  /* with REC_PIDS: the frame passes pids_frame_push's CRC-12 (pids.c:52-86), i.e. sis_decode will see it */
    NRSC5HIP_REC_DISCARDED = 1u << 10  /* internal (p1_async + l2_feedback): a block that ran speculatively behind a P1 frame whose first L2 header
                                          failed; the stream was rewound to that frame.  nrsc5hip_drain / _batch_fetch* never deliver such records */
};

/* One record per processed 32-symbol block, in stream order.  Events implied by one record fire in
 * the order of the flag bits above (which is the reference's order inside acquire_process). */
typedef struct nrsc5hip_record {
    uint32_t flags;
    int32_t state_before, state_after;   /* sync state entering / leaving the block */
    int32_t samperr;                     /* timing pick used for this block, 0..2159 (acquire.c:112,149) */
    int32_t cfo;                         /* integer carrier offset in bins after this block */
    int32_t keep;                        /* samples carried to the next window (acquire.c:259) */
    int32_t bc;                          /* block count after this block */
    int32_t psmi;
    int32_t cfo_wait;
    int32_t next_samperr;                /* tracking feedback for the next block (sync.c:455) */
    float prev_angle;                    /* CP-lag phase estimate, rad per 2048 samples */
    float phase_re, phase_im;            /* NCO phase after the block */
    float next_angle;                    /* residual CFO feedback (sync.c:458) */
    float freq_offset;                   /* Hz, valid with REC_TO_FINE (input.c:181-184) */
    float mer_lb, mer_ub;                /* dB, valid with REC_MER */
    float ber;                           /* valid with REC_P1 */
    int32_t p1_slot;                     /* valid with REC_P1 */
    int32_t bc_decoded;                  /* block count the PIDS frame / soft bits belong to, or -1 */
    uint32_t pids[3];                    /* valid with REC_PIDS: bit i of the frame at pids[i/32] bit i%32 */
    uint32_t sis;                        /* AM with REC_TO_FINE: pli | hppi << 1 | aabi << 2 | rdbi << 3 | 16 (sync.c:231-235);
                                            FM with REC_P3 / REC_P4: slot of the P3/P4 frame ring (8 * p1_slots slots) */
} nrsc5hip_record;

typedef struct nrsc5hip_config {
    int device;                /* HIP device ordinal */
    int max_streams;           /* independent IQ streams resident in this engine */
    long long q15_capacity;    /* decimated (744187.5 S/s) samples of FIFO per stream; >= 2 * 71280.
                                  Batch use: capture length / 2 + 64 for a capture appended whole; a session of any length that
                                  trims (nrsc5hip_batch_trim) needs NRSC5HIP_TRIM_RETAIN_MAX + its largest append. */
    int record_capacity;       /* block records retained per stream between drains (>= 64) */
    int p1_slots;              /* decoded P1 frames retained per stream between drains (>= 2) */
    int p1_async;              /* 0: decode each P1 frame before the next block of any stream (exact
                                  reference event timing; required for nrsc5hip_force_resync feedback);
                                  1: decode the frames of each 16-block window on a second HIP stream,
                                  overlapped with the next window (throughput mode) */
    int l2_feedback;           /* 1: the engine itself applies the L2 -> L1 feedback of frame_process (frame.c:516-540): a P1 frame
                                  whose first L2 header fails the RS(255,247) check drops the stream to SYNC_NONE (REC_LOST_SYNC)
                                  before its next block, as in the reference.  With p1_async = 1 (FM and AM) the verdict of a deferred
                                  decode arrives windows later: the stream is then rewound to the end of the block that delivered the
                                  frame and re-run from there, so the delivered records and frames are the reference's all the same
                                  (the samples since that block stay in the FIFO: the batch appends never discard any, and
                                  nrsc5hip_batch_trim gives back only what lies in front of every checkpoint a verdict may still
                                  rewind to, so a batch session may run for any length; streaming pushes: drain the records after
                                  each call; and record_capacity >= 256).
                                  0: the host does it through nrsc5hip_force_resync (the drop-in shim). */
    int am_enable;             /* allocate the AM buffers (1.4 MB per stream) so that streams may be switched to
                                  NRSC5HIP_MODE_AM */
    int batch_zero_copy;       /* 1: nrsc5hip_batch_append_cu8 on freshly reset FM streams does NOT decimate into the FIFO: the engine keeps a
                                  reference to the caller's device buffer and the block steps read the cu8 samples directly (half-band
                                  fused into the symbol kernel: the capture is read from HBM once, no 4-byte-per-sample Q15 copy).
                                  The buffer must stay valid and unchanged until those streams are reset; one append per stream and
                                  reset; q15_capacity may then be the minimum (2 * 71280).  0: samples are copied (decimated) into the
                                  engine's FIFO during the call, as the streaming seam does. */
    int l2_index;              /* 1: every FM P1 frame is also indexed on the decode stream right after its traceback
                                  (nrsc5hip_l2_frame per ring slot, read with nrsc5hip_l2_frame_get / nrsc5hip_batch_fetch_l2), and
                                  so are the P3 / P4 frames and the frames of AM streams (nrsc5hip_batch_fetch_l2_px / _am);
                                  0: indexes only on request (nrsc5hip_l2_index) */
} nrsc5hip_config;

typedef struct nrsc5hip_engine nrsc5hip_engine;

/* Devices and threads.  An engine lives on cfg.device; EVERY entry point that takes an engine switches the calling thread to that
 * device for the duration of the call and restores the thread's previous current device on return, so one process may own one
 * engine per GPU (integration/batch_shard.c: N host threads x one engine per visible GPU) whatever hipSetDevice the caller last
 * made.  An engine is NOT re-entrant: at most one thread may be inside calls on the SAME engine at a time (give each thread its
 * own engine, or serialise); different engines -- on the same or on different devices -- may be driven concurrently from different
 * threads: nothing is shared between engines (no process-global scratch, per-thread error string and seam counters).
 * nrsc5hip_last_error() returns the calling thread's last message.  Device pointers handed to the batch entry points must belong
 * to the engine's device.  The window pipeline (p1_async = 1) needs GPU_MAX_HW_QUEUES >= 8 in the environment before the HIP runtime
 * initialises (one hardware queue per chain / decode stream); engine creation warns on stderr when it is lower. */
int nrsc5hip_engine_create(const nrsc5hip_config *cfg, nrsc5hip_engine **out);
void nrsc5hip_engine_destroy(nrsc5hip_engine *e);
const char *nrsc5hip_last_error(void);
/* fingerprint of the device sources this library was built from (nrsc5_amd/build.py: source_sha) -- measurements are only taken
 * with a library that matches the tree */
const char *nrsc5hip_source_sha(void);
/* hipStream_t the engine launches on, as void* (so that callers can order their own work) */
void *nrsc5hip_engine_hip_stream(nrsc5hip_engine *e);

/* Device helpers for hosts that do not link the HIP runtime themselves: number of visible GPUs; a device buffer on `device` filled
 * from host memory (host may be NULL: allocation only); its release.  The pointers are what the batch entry points take. */
int nrsc5hip_device_count(int *n);
int nrsc5hip_device_upload(int device, const void *host, size_t nbytes, void **dev_out);
int nrsc5hip_device_free(int device, void *dev);

/* ---- streaming seam (host buffers), one stream at a time --------------------------------------- */
/* input_push_cu8 (input.c:96-117): nbytes % 4 == 0.  Decimates, appends, and processes every block
 * whose 33-symbol window is complete; records are then available through nrsc5hip_drain.  With p1_async = 0 the host keeps a
 * mirror of the stream's read position.  FM cu8 (round 6, NRSC5HIP_TUNE_HOST_CAPTURE): the bytes stay, as pushed, in a pinned device-mapped capture
 * that the stream reads in place -- a push that completes no block is ONE host memcpy and nothing else; the block step is the symbol kernel
 * (half-band fused, loading across PCIe) + the sync kernel, which posts the block's record into pinned host memory itself.  Other input (cs16, AM,
 * or with the knob at 0): a push that completes no block is one memcpy into pinned staging + the decimator launch (no synchronisation).  Either way a
 * push that completes a block ends with the host spinning on the report's sequence number, the block's record already in host memory. */
int nrsc5hip_push_cu8(nrsc5hip_engine *e, int stream, const uint8_t *iq, uint32_t nbytes);
/* input_push_cs16 (input.c:119-124): n = number of int16 values, n % 2 == 0 */
int nrsc5hip_push_cs16(nrsc5hip_engine *e, int stream, const int16_t *iq, uint32_t n);
/* input_reset (input.c:126-138) on a session that may have been used: like the reference's, the reset rewinds the FIR windows without clearing them
 * (firdecim_q15_reset, firdecim_q15.c:53-56) -- the first 7 samples out of the FM half-band and the acquisition filter's first 31 outputs (filter_fm or
 * filter_am, acquire.c:290-293) see the samples the window's last compaction left at its front, exactly as a second capture on one nrsc5_t does
 * (tests: engine_checks.check_reset_keeps_fir_windows vs the unmodified reference).  Bytes of a partial push still staged on the host pass through the
 * decimator first.  The five stages of the AM cu8 cascade (input.c:70-88) are covered as well, and so is what sync_reset (sync.c:810-830) leaves alone:
 * sync_t.samperr, .angle and .bc keep their values -- visible in the block records of the next capture's un-synchronised blocks, and, because the AM path never
 * writes .angle, in the angle of the first synchronised block of an AM session that follows an FM one (acquire.c:115-118).  A LOST_SYNC that the reference
 * fires inside the reset (input_set_sync_state) is the caller's own doing and no record.  Engines with batch_zero_copy treat every reset as a fresh session. */
int nrsc5hip_stream_reset(nrsc5hip_engine *e, int stream);
/* ABI NOTE (NRSC5HIP_ABI_VERSION >= 5): until round 4 nrsc5hip_stream_reset gave a FRESH session; since round 5 it is the reference's input_reset as described above (stale FIR
 * windows, samperr / angle / bc kept) and the fresh session is nrsc5hip_stream_fresh.  A caller that used reset to start an independent capture on a slot must call
 * nrsc5hip_stream_fresh now (on engines with batch_zero_copy both are the fresh form).  nrsc5hip_abi_version() lets a binding check what it was linked against. */
#define NRSC5HIP_ABI_VERSION 24   /* 24: + reception impairments of the analog host (nrsc5hip_fm_impair_enable, nrsc5hip_fm_impair, nrsc5hip_fm_impair_taps, nrsc5hip_stage_fm_impair); 23: + EAS alerts (SAME) of the analog host (nrsc5hip_fm_same_enable, _same_read, _same_get, _same_stats, _same_info, _same_table, nrsc5hip_stage_same_tones, _stage_same_frames); 22: + reception steering of the analog FM audio (nrsc5hip_fm_steer_enable, nrsc5hip_fm_steer, nrsc5hip_fm_steer_taps, nrsc5hip_stage_fm_steer); 21: + carrier quality of the analog host (nrsc5hip_fm_carrier_enable, nrsc5hip_fm_carrier, nrsc5hip_stage_fm_carrier) and the analog-carrier detector (nrsc5hip_scan_detect_fm_psd, nrsc5hip_scan_detect_fm); 20: + nrsc5hip_stage_symbols; 19: + RDS of the analog host (nrsc5hip_fm_rds_*, nrsc5hip_stage_rds_mf, _stage_rds_groups), nrsc5hip_fm_debug_launches; 18: + nrsc5hip_stage_am_block, nrsc5hip_debug_fetch_am_sym; 17: + nrsc5hip_stage_nco_exact; 16: + analog FM audio (nrsc5hip_fm_*, nrsc5hip_stage_fm_mpx, nrsc5hip_chan_feed_fm); 15: + the data services (nrsc5hip_aas_*, nrsc5hip_stage_aas, _stage_aas_frames); 14: + SIS on the device (nrsc5hip_sis_*, nrsc5hip_stage_sis); 13: + the coarse-acquisition stage hooks (nrsc5hip_stage_acquire, _acquire_raw, _am_acquire); 12: + the PSD transport (nrsc5hip_psd_*, nrsc5hip_stage_psd); 11: + nrsc5hip_hdc_feed; 10: + nrsc5hip_batch_trim, NRSC5HIP_TRIM_RETAIN_MAX; 9: + the band scan (nrsc5hip_scan_*); 8: + the wideband channelizer (nrsc5hip_chan_*); 7: + NRSC5HIP_TUNE_HOST_CAPTURE / _FOLD_REPORT, nrsc5hip_debug_host_capture_stats; 6: + nrsc5hip_abi_version, nrsc5hip_debug_flow_stats, NRSC5HIP_TUNE_FLOW_MIN / _LOOP_EXACT, NRSC5HIP_PROF_FLOW; 5: the reset semantics above */
int nrsc5hip_abi_version(void);
/* nrsc5_close + nrsc5_open_pipe on this slot: a fresh session (calloc'd windows), what nrsc5hip_reset_all does for every stream */
int nrsc5hip_stream_fresh(nrsc5hip_engine *e, int stream);
/* nrsc5_set_mode -> input_set_mode (nrsc5.h:754, input.c:158-162): NRSC5HIP_MODE_FM (default) or _AM; resets the stream.
 * AM: cu8 pushes go through the 5-stage 32:1 decimator, cs16 pushes are 46511.71875 S/s samples (input.c:70-91,119-124);
 * every FINE block yields a PIDS frame and (after the 4-frame diversity start-up) one 3750-bit P1 frame, block 7 also the
 * P3 frame and the BER.  Event order inside an AM record: TO_FINE, PIDS, P1 frame, P3 frame, BER (decode.c:507-554). */
int nrsc5hip_stream_set_mode(nrsc5hip_engine *e, int stream, int mode);
/* L2 feedback (frame.c:535-540): the stream drops to SYNC_NONE before its next block */
int nrsc5hip_force_resync(nrsc5hip_engine *e, int stream);
/* Input bytes of this format (cu8 != 0: cu8, else cs16) whose push completes the stream's next 32-symbol block.  A caller that
 * applies the L2 feedback itself (frame.c through nrsc5hip_force_resync: the drop-in) pushes at most this much per call, so the
 * frames of one block reach L2 before the next block is processed -- the reference's event order for any push size.  -1: not
 * known (p1_async engines, or a stream that the batch entry points touched since its reset): push <= 17280 bytes per call. */
long long nrsc5hip_bytes_to_next_block(nrsc5hip_engine *e, int stream, int cu8);
/* Deferred wait (p1_async = 0).  A block that starts in SYNC_FINE consumes a number of samples the host can compute from the
 * previous block's record (keep = 2160 - next_samperr, acquire.c:112,259), so the push that completes such a block returns with
 * the block step still running: the device works on block n while the caller reads and pushes the samples of block n + 1.
 * nrsc5hip_bytes_to_next_block stays exact.  Every other entry point (nrsc5hip_drain first of all) waits for the step before it
 * does anything, so a caller that never heard of this sees the old behaviour; a caller that wants the overlap polls with
 * nrsc5hip_drain_ready, which hands out what has been reported so far and never waits.
 *
 * Manual stepping lets the L2 feedback of block n (frame.c -> nrsc5hip_force_resync) reach the engine before block n + 1 is
 * STEPPED while the samples of block n + 1 are already in the capture / on their way into the FIFO: with it set, a push that completes a block
 * copies (or submits) the samples and returns; the caller then drains block n (nrsc5hip_drain, waits), feeds L2, and calls
 * nrsc5hip_stream_step.  integration/input_hip.c does exactly that.  (A push that finds an unstepped complete block steps it
 * itself: forgetting the call costs speed, never samples.) */
int nrsc5hip_drain_ready(nrsc5hip_engine *e, int stream, nrsc5hip_record *out, int max, int *n_out);
int nrsc5hip_stream_set_manual_step(nrsc5hip_engine *e, int stream, int on);
int nrsc5hip_stream_step(nrsc5hip_engine *e, int stream);
/* One step further: when the block step still in flight started in SYNC_FINE and cannot complete a P1 frame (15 of 16 blocks), nothing
 * its delivery tells the host can change what the next block does -- frame_process's only way back into L1 is the first header of a
 * P1 frame (frame.c:535-540) -- so the next block's step may be queued BEHIND it before the host has even looked at it:
 * nrsc5hip_stream_step_ahead does that if it is safe and says so in *submitted; the nrsc5hip_drain that follows waits for the older
 * step only.  The device then runs block n + 1 while the host hands block n to L2.
 * CONTRACT: between a nrsc5hip_stream_step_ahead that reported *submitted = 1 and the nrsc5hip_drain that follows it, the caller must not issue
 * anything that changes the stream's L1 state (nrsc5hip_force_resync, nrsc5hip_stream_reset, nrsc5hip_stream_set_mode): the block queued ahead has
 * already been submitted with the old state, so the change would land one block late.  (integration/input_hip.c cannot violate it: those calls
 * only come from frame.c during a delivery, and a delivery that can produce them -- a block that may end a P1 frame -- is never stepped ahead of.)
 * Should the engine find its own prediction violated (a block submitted without its P1 decode completed a frame while the next one is running)
 * it drops both steps' bookkeeping, marks the stream's host mirror invalid (the next push re-synchronises) and returns NRSC5HIP_EHIP.  The events of those two
 * blocks are then NOT delivered through the seam (their records remain in the device ring for nrsc5hip_drain; the first block's P1 frame has no decode): the
 * session has failed and says so -- it never continues silently. */
int nrsc5hip_stream_step_ahead(nrsc5hip_engine *e, int stream, int *submitted);
/* EVENT LATENCY of the drop-in built on these calls (integration/input_hip.c; INTEGRATION.md, first section).  DEFAULT since round 6: the shim waits inside the call that
 * completes a block and delivers that block's events before it returns -- the reference's contract (src/input.c:41-50).  With NRSC5HIP_OVERLAP_DELIVERY=1 (deferred waits,
 * steps queued ahead: ~1.5 x the throughput) the records of block n reach the caller during the first call after the device has finished it -- at the latest in the call
 * that completes block n + 1, i.e. up to one block (92.9 ms of signal) later than src/input.c fires them -- or in a zero-length push (flush), nrsc5hip_drain (waits),
 * stream reset / engine destruction paths of the shim. */

/* ---- batch path (device buffers) ------------------------------------------------------------------ */
/* Decimate + append one cu8 chunk per listed stream.  dev_iq: device pointer, chunk k at
 * dev_iq + k * stride_bytes (16-byte aligned), nbytes[k] bytes each (host array, % 4 == 0). */
int nrsc5hip_batch_append_cu8(nrsc5hip_engine *e, int nstreams, const int *stream_ids,
                              const uint8_t *dev_iq, long long stride_bytes, const uint32_t *nbytes);
int nrsc5hip_batch_append_cs16(nrsc5hip_engine *e, int nstreams, const int *stream_ids,
                               const int16_t *dev_iq, long long stride_elems, const uint32_t *nelems);
/* An append that does not fit (retained samples + new ones > q15_capacity) fails with NRSC5HIP_EOVERFLOW and leaves every listed stream untouched:
 * the appends never discard samples by themselves.  Space comes back through nrsc5hip_batch_trim (ABI 10):
 *
 * Give back the FIFO space of the listed streams that nothing can read again: everything before min(rd, the oldest checkpoint a pending
 * first-header verdict may rewind to).  retained[k] (may be NULL) = samples stream k still holds (wr - base) afterwards.
 * The live samples move to the front of the stream's slab on the engine's stream, behind every block step and rollback submitted so far and ahead of the
 * next append; results (records, frames) are the same as without the call.  Streams that read a capture in place (batch_zero_copy appends, the pinned
 * capture of the fast streaming seam) hold nothing in the FIFO: they are left alone and report 0.  A stream id listed twice is NRSC5HIP_EINVAL.  A stream of the streaming seam that is listed here
 * is, as with every batch entry point, read from the device from then on.
 *
 * NRSC5HIP_TRIM_RETAIN_MAX bounds what a trim can retain for a stream whose complete blocks have all been processed (nrsc5hip_batch_process ran until
 * nothing was left): the oldest checkpoint with an open verdict belongs to a frame at most NWIN = 8 decode windows of 16 blocks old -- the decode of window w
 * is waited for, and its verdict taken, before window w + 8 reuses its slot; NRSC5HIP_TUNE_VERDICT_LAG is clamped to 8 windows and so adds nothing -- and a
 * block step advances the read position by at most its 33-symbol window of 71280 samples; the block in progress (the unread tail) is less than one more
 * window.  (This bound is conservative by design.  With the present scheduler every nrsc5hip_batch_process, also one that stops at max_steps, returns with
 * every deferred decode finished and every verdict taken, so the floor of a trim between two calls is the read position itself and the checkpoint terms
 * never apply: the retained span measured after a process call that ran to the end is under one window, 71280 samples.  The bound, and with it a least
 * capacity of 36.8 MB per station, is what the rule guarantees without relying on that.)  AM streams: windows of 8 blocks of 8910 samples each, NRSC5HIP_TRIM_RETAIN_MAX_AM.  Between two nrsc5hip_batch_process calls that ran to the end every verdict
 * has been taken, and a trim then retains less than one window.  The smallest q15_capacity that carries a session of any length is therefore
 * NRSC5HIP_TRIM_RETAIN_MAX (_AM for an AM stream) + the largest single append (in decimated samples); when the retained span leaves less room than that, the append reports
 * NRSC5HIP_EOVERFLOW with the retained span in its message -- samples are never dropped silently. */
#define NRSC5HIP_TRIM_RETAIN_MAX    ((8LL * 16 + 1) * 71280)  /* 9 195 120 samples (36.8 MB per stream) */
#define NRSC5HIP_TRIM_RETAIN_MAX_AM ((8LL * 8 + 1) * 8910)    /*   579 150 samples */
int nrsc5hip_batch_trim(nrsc5hip_engine *e, int nstreams, const int *stream_ids, long long *retained);
/* Run block steps (every listed stream advances by at most one block per step) until no listed stream
 * has a complete window or max_steps is reached; *steps_done gets the number of steps that did work. */
int nrsc5hip_batch_process(nrsc5hip_engine *e, int nstreams, const int *stream_ids, int max_steps, int *steps_done);

/* ---- results ----------------------------------------------------------------------------------------- */
/* Copies up to max records of `stream`, oldest first, that were produced since the previous drain. */
int nrsc5hip_drain(nrsc5hip_engine *e, int stream, nrsc5hip_record *out, int max, int *n_out);
/* P1 frame of a REC_P1 record, packed (bit i at words[i/32] bit i%32) ... */
int nrsc5hip_p1_frame_packed(nrsc5hip_engine *e, int stream, int slot, uint32_t *words /* [4568] */);
/* ... or one bit per byte, the layout frame_push() takes (frame.h:53) */
int nrsc5hip_p1_frame_bits(nrsc5hip_engine *e, int stream, int slot, uint8_t *bits /* [146176] */);
/* FM extended sidebands (decode_push_px1/px2, decode.c:393-437): P3 (channel 0) / P4 (channel 1) frame of a REC_P3 / REC_P4
 * record, slot = record.sis, nbits = 2304 (MP2) or 4608 (MP3 / MP11), one bit per byte as frame_push() takes it */
int nrsc5hip_px_frame_bits(nrsc5hip_engine *e, int stream, int slot, int channel, int nbits, uint8_t *bits);
/* every P3/P4 slot of the listed streams, packed: frames[nstreams][8 * p1_slots][2][144] */
int nrsc5hip_batch_fetch_px(nrsc5hip_engine *e, int nstreams, const int *stream_ids, uint32_t *frames);
/* AM frames of a REC_P1 / REC_P3 record, one bit per byte as frame_push() takes them: which = 0..7 selects the P1 frame
 * of that block (nbits 3750), which = 8 the P3 frame (nbits 24000 for MA1, 30000 for MA3).  In the packed slot
 * (nrsc5hip_p1_frame_packed / batch_fetch) P1 frame b starts at word 118 b and the P3 frame at word 944. */
int nrsc5hip_am_frame_bits(nrsc5hip_engine *e, int stream, int slot, int which, int nbits, uint8_t *bits);
/* Bulk D2H of every record/frame produced by a batch: records[nstreams][max_records],
 * counts[nstreams]; frames may be NULL, else frames[nstreams][p1_slots][4568] */
int nrsc5hip_batch_fetch(nrsc5hip_engine *e, int nstreams, const int *stream_ids, nrsc5hip_record *records,
                         int max_records, int *counts, uint32_t *frames);
/* Zero-copy variant for streams 0..nstreams-1: bulk D2H into engine-owned pinned buffers; *records points at
 * [nstreams][record_capacity] records, *frames (may be NULL) at [nstreams][p1_slots][4568] words; valid until the
 * next fetch / reset.  Requires an undrained, unwrapped record ring (batch use after nrsc5hip_reset_all). */
int nrsc5hip_batch_fetch_view(nrsc5hip_engine *e, int nstreams, const nrsc5hip_record **records, int *counts, const uint32_t **frames);
/* unpack helper (host only) */
void nrsc5hip_unpack_bits(const uint32_t *words, int nbits, uint8_t *bits);

/* ---- L2 audio transport index (frame.c:516-714), an additive post-pass over decoded frames that are still in HBM ----
 * frame_push (PCI extraction, bit order) and the audio walk of frame_process run on the device: every audio PDU's
 * RS(255,247)-corrected header, its locators, header expansion fields, PSD span and the CRC-8 verdict of each packet,
 * i.e. what frame_process hands to output_align / parse_hdlc / output_push, as offsets into the frame's PDU bytes.
 * A host that takes the index need not touch the 146 176 bits of a P1 frame one by one (frame.c:688-709). */
#define NRSC5HIP_L2_MAX_PDUS     16
#define NRSC5HIP_L2_MAX_PACKETS  64      /* MAX_AUDIO_PACKETS, frame.c:30 */
#define NRSC5HIP_L2_MAX_BYTES    18269   /* MAX_PDU_LEN, defines.h:63 */
enum {                                   /* nrsc5hip_l2_frame.status: why the walk ended */
    NRSC5HIP_L2_END = 0,                 /* ran to the end of the frame (frame.c:525) */
    NRSC5HIP_L2_NO_AUDIO,                /* !has_audio (frame.c:522) */
    NRSC5HIP_L2_FIXED_DATA,              /* (unused since round 2: frames with fixed-data sub-channels ARE indexed, with audio_end = nbytes - 1, the
                                            largest value process_fixed_data can return; the consumer cuts the index back with the true value:
                                            nrsc5hip_l2_apply_audio_end, done inside nrsc5hip_hdc_push_frame) */
    NRSC5HIP_L2_HEADER_RS,               /* fix_header failed (frame.c:534-541); lost_sync tells whether this drops the receiver to SYNC_STATE_NONE */
    NRSC5HIP_L2_BAD_LOCATORS,            /* one of the returns of frame.c:547-556 (typical: zero padding after the last PDU) */
    NRSC5HIP_L2_TOO_MANY_PDUS,           /* more than NRSC5HIP_L2_MAX_PDUS audio PDUs */
    NRSC5HIP_L2_HEF_OVERRUN,             /* header expansion runs past la_location: the reference's parse_hdlc length wraps (undefined) */
    NRSC5HIP_L2_BAD_STREAM,              /* stream_id >= MAX_STREAMS with nop == 0: the reference reads locations[-1] */
    NRSC5HIP_L2_BAD_LENGTH,              /* not one of frame_push's six frame lengths (frame.c:683) */
    NRSC5HIP_L2_AUDIO_END                /* set by nrsc5hip_l2_apply_audio_end: the walk ended where the fixed-data region begins (frame.c:525,547-556) */
};
/* PCI values that announce fixed-data sub-channels next to audio (has_fixed && has_audio, frame.c:138-151) */
#define NRSC5HIP_L2_PCI_HAS_FIXED(pci) ((((pci) & 0xFFFFFCu) == (0xE3634Cu & 0xFFFFFCu)) || (((pci) & 0xFFFFFCu) == (0x8D8D33u & 0xFFFFFCu)))
typedef struct nrsc5hip_l2_pdu {
    uint32_t start;                      /* offset of the PDU (its RS parity bytes) in the frame's PDU bytes */
    uint32_t psd_off; int32_t psd_len;   /* the span frame_process gives parse_hdlc (frame.c:611) */
    uint32_t audio_off;                  /* first byte of packet 0 = start + la_location + 1 */
    uint32_t crc_bad_lo, crc_bad_hi;     /* bit j: packet j fails its CRC-8 (PACKET_FLAG_CRC_ERROR, frame.c:616-627) */
    uint32_t pdu_marker;                 /* HEF class 4 */
    uint16_t hef_pdu_len;                /* HEF class 1 */
    uint16_t loc[NRSC5HIP_L2_MAX_PACKETS]; /* offset of packet j's CRC byte; packet j = [loc[j-1] + 1 (audio_off for j = 0), loc[j]) */
    uint8_t codec_mode, stream_id, pdu_seq, blend_control, per_stream_delay, common_delay, latency, pfirst, plast, seq, nop,
            hef, la_location;            /* parse_header, frame.c:181-196 */
    uint8_t rs_corrections;              /* symbols fix_header corrected in this header */
    uint8_t class_ind, prog_num, access, prog_type, applied_services;   /* parse_hef, frame.c:198-265 */
    uint8_t elastic_seq;                 /* `seq` of packet 0 in the elastic buffer, frame.c:593 */
    uint8_t align_offset;                /* output_align's offset, frame.c:595-600 */
    uint8_t skipped;                     /* stream_id >= MAX_STREAMS: packets skipped as frame.c:559-564 does */
} nrsc5hip_l2_pdu;
typedef struct nrsc5hip_l2_frame {
    uint32_t pci;                        /* protocol control information bits, frame.c:695-699 */
    uint32_t nbytes;                     /* PDU bytes of the frame */
    uint32_t n_pdu, status;
    uint32_t end_offset;                 /* where the walk stopped */
    uint32_t lost_sync;                  /* 1: frame_process calls input_set_sync_state(SYNC_STATE_NONE) on this frame (frame.c:537-538) */
    nrsc5hip_l2_pdu pdu[NRSC5HIP_L2_MAX_PDUS];
} nrsc5hip_l2_frame;
enum { NRSC5HIP_L2_FM_P1 = 0, NRSC5HIP_L2_FM_PX = 1, NRSC5HIP_L2_AM = 2 };
typedef struct nrsc5hip_l2_job {
    int32_t stream, slot;                /* as for nrsc5hip_p1_frame_bits / _px_frame_bits / _am_frame_bits */
    int32_t kind;                        /* NRSC5HIP_L2_FM_P1 | _FM_PX (which = channel) | _AM (which = 0..7 P1 of that block, 8 = P3) */
    int32_t which, nbits;                /* nbits: 146176 | 2304 / 4608 | 3750 / 24000 / 30000 */
} nrsc5hip_l2_job;
/* Index njobs decoded frames in one launch.  out[njobs]; pdu_bytes may be NULL, else job k's PDU bytes (RS-corrected
 * headers) go to pdu_bytes + k * stride (stride >= (nbits - pci bits) / 8).  Host buffers. */
int nrsc5hip_l2_index(nrsc5hip_engine *e, int njobs, const nrsc5hip_l2_job *jobs, nrsc5hip_l2_frame *out,
                      uint8_t *pdu_bytes, long long stride);
/* engine option l2_index: the index computed in the pipeline for the FM P1 frame in `slot` (the slot a REC_P1 record names) */
int nrsc5hip_l2_frame_get(nrsc5hip_engine *e, int stream, int slot, nrsc5hip_l2_frame *out);
/* ... and of every P1 slot of the listed streams: out[nstreams][p1_slots] */
int nrsc5hip_batch_fetch_l2(nrsc5hip_engine *e, int nstreams, const int *stream_ids, nrsc5hip_l2_frame *out);
/* The same option also indexes, in the pipeline, the P3 / P4 frames of the extended sidebands -- out[nstreams][px_slots = 8 *
 * p1_slots][2], entry [slot][0] = the P3 frame a REC_P3 record names in `sis`, [slot][1] its P4 frame (MP11) -- and, in engines
 * created with am_enable, the frames of every AM L1 frame slot: out[nstreams][p1_slots][9], entries 0..7 = the P1 frame delivered
 * at block 0..7 (REC_P1, p1_slot), 8 = the P3 frame (REC_P3).  Entries of slots no record names are stale or zero. */
int nrsc5hip_batch_fetch_l2_px(nrsc5hip_engine *e, int nstreams, const int *stream_ids, nrsc5hip_l2_frame *out);
int nrsc5hip_batch_fetch_l2_am(nrsc5hip_engine *e, int nstreams, const int *stream_ids, nrsc5hip_l2_frame *out);
/* stage-level twin: nframes logical frames given as frame_push takes them (one bit per byte, nbits each) */
int nrsc5hip_stage_l2_index(nrsc5hip_engine *e, const uint8_t *bits, int nbits, int nframes, nrsc5hip_l2_frame *out,
                            uint8_t *pdu_bytes, long long stride);

/* ---- batch HDC hand-off (host side) --------------------------------------------------------------------
 * The reference keeps a 22.9 MB nrsc5_t per session, 18.7 MB of it the elastic buffers of output_t (output.h:104-122).  A
 * batch of 2048 streams cannot; this consumer keeps ~40 KB per stream and program and reproduces, from the L2 index
 * (nrsc5hip_l2_frame + the PDU bytes nrsc5hip_l2_index returns), exactly the NRSC5_EVENT_HDC sequence of the reference:
 *   nrsc5hip_hdc_push_frame = frame_process's output_align / output_push calls for one frame   (frame.c:590-640, output.c:31-92)
 *   nrsc5hip_hdc_advance    = output_advance: call it once per block record (NRSC5HIP_REC_PROCESSED), BEFORE handing over
 *                             the frames that record announces, as acquire.c:108 does; every complete packet goes to `cb`
 *                             with the event's fields (program, data, count, flags; nrsc5.c:709-728).  Returns the count.
 *   nrsc5hip_hdc_adts       = dump_hdc's framing (main.c:182-212): 7-byte ADTS header + payload into out[count + 7]
 * No device work: plain host functions, usable from any thread (one consumer object per thread). */
typedef struct nrsc5hip_hdc nrsc5hip_hdc;
typedef void (*nrsc5hip_hdc_cb)(void *opaque, int stream, unsigned program, const uint8_t *data, unsigned count, unsigned flags);
int nrsc5hip_hdc_create(int nstreams, nrsc5hip_hdc **out);
void nrsc5hip_hdc_destroy(nrsc5hip_hdc *h);
int nrsc5hip_hdc_reset(nrsc5hip_hdc *h, int stream);                 /* output_reset (output.c:204-218) */
/* lc: logical channel of the frame (0 = P1, 1 = P3, 2 = P4), which selects the fixed-data (CCC) state it advances */
int nrsc5hip_hdc_push_frame(nrsc5hip_hdc *h, int stream, int lc, const nrsc5hip_l2_frame *ix, const uint8_t *pdu_bytes);
/* frames with fixed-data sub-channels: process_fixed_data's audio_end for this frame (frame.c:458-514: sync-byte tracking,
 * CCC HDLC frames, sub-channel lengths) -- advances the stream's CCC state; and the cut of an index that was built with
 * audio_end = nbytes - 1 back to it (the loop / locator conditions of frame.c:525,547-556).  nrsc5hip_hdc_push_frame calls both
 * for such frames; they are exported for consumers that keep their own elastic buffers.  apply returns the PDUs kept, or -1
 * when a header expansion ran into the fixed-data region (the reference's parse is cut there: walk that frame on the host). */
unsigned nrsc5hip_hdc_fixed_audio_end(nrsc5hip_hdc *h, int stream, int lc, const uint8_t *pdu_bytes, unsigned nbytes);
int nrsc5hip_l2_apply_audio_end(nrsc5hip_l2_frame *ix, unsigned audio_end);
/* sync.c:405-409: frame_reset when a stream enters FINE (NRSC5HIP_REC_TO_FINE) clears the CCC state; the elastic buffers stay */
int nrsc5hip_hdc_frame_reset(nrsc5hip_hdc *h, int stream);
int nrsc5hip_hdc_advance(nrsc5hip_hdc *h, int stream, int mode /* NRSC5HIP_MODE_FM | _AM */, nrsc5hip_hdc_cb cb, void *opaque);
size_t nrsc5hip_hdc_adts(const uint8_t *data, unsigned count, uint8_t *out);
size_t nrsc5hip_hdc_host_bytes(const nrsc5hip_hdc *h);                /* host memory held by the consumer */
/* Replays block records of `nstreams` engine streams into the consumer, stream by stream, in the reference's order:
 * output_advance at the top of every processed block, the frame reset on a transition to fine sync, then every logical frame the
 * block delivers (FM: P1, P3, P4; AM: the P1 PDUs and P3), each through frame_process's path (nrsc5hip_hdc_push_frame).  ONE L2
 * index launch and one copy for all frames of the call.  targets[i] is the consumer's stream for stream_ids[i] (NULL: the same
 * ids).  records[i] / counts[i]: the records of stream_ids[i] as nrsc5hip_drain / _batch_fetch delivered them, in order; a session
 * may be fed in as many calls as it likes.  Must be called while the frame ring slots the records name still hold their frames (the
 * contract of nrsc5hip_p1_frame_bits).  A loss of sync (NRSC5HIP_REC_LOST_SYNC) changes nothing in the consumer, as it changes
 * nothing in the reference's output_t: packets already pushed keep coming out, block by block, while the stream re-acquires.
 * Packets are delivered through cb (may be NULL: count only) inside the call, all of stream_ids[0] first, then stream_ids[1], ...;
 * returns the number of packets delivered or a negative error.  nstreams == 0 or all counts zero: 0, nothing delivered.  Ids out
 * of range (engine or consumer), a NULL records[i] with counts[i] > 0 and a mode that is neither FM nor AM are NRSC5HIP_EINVAL
 * and leave the consumer untouched; so does a record that names a slot the engine does not have, or a failure of the index launch
 * or its copy.  Behind that point the call is NOT atomic: the replay can still fail on a frame whose header expansion runs into the
 * fixed-data region (nrsc5hip_hdc_push_frame's NRSC5HIP_EINVAL, see nrsc5hip_l2_apply_audio_end), and the call then returns that
 * error with the records in front of the frame replayed and their packets already delivered through cb; the packet count is lost.
 * Walk such a frame on the host, or nrsc5hip_hdc_reset the stream. */
int nrsc5hip_hdc_feed(nrsc5hip_hdc *h, nrsc5hip_engine *e, int nstreams, const int *stream_ids, const int *targets,
                      const nrsc5hip_record *const *records, const int *counts, int mode, nrsc5hip_hdc_cb cb, void *opaque);

/* ---- PSD transport: now-playing text without the audio payload (device side: csrc/k_psd.hip) ---------------------------------
 * Program service data travels as an HDLC byte stream cut across the audio PDUs of each program; the reference reassembles it in
 * parse_hdlc / aas_push (frame.c:328-391, 611) into AAS packets, of which ports 0x5100 and 0x5201..0x5207 carry ID3 tags
 * (output.c:874-882).  This consumer does that on the device, over the L2 index and the RS-corrected PDU bytes of the frames the records
 * name, which stay in HBM: per (consumer stream, program 0..7) it keeps frame_t.psd_buf / psd_idx (8212 bytes and an index, -1 = closed;
 * 66 KB per stream) in device memory, and only finished packets are copied to the host.
 * Rules, each equal to the reference's: bytes [psd_off, psd_off + psd_len) of every PDU the walk keeps (skipped == 0), whatever its
 * stream_id or logical channel, go to the state of its prog_num -- P1, P3, P4 and AM frames of one stream share the eight states.  0x7E
 * closes the open frame (if one is open) and opens the next; any other byte is stored while the frame is open and shorter than 8212 raw
 * bytes, the byte that finds it full closes it unseen (overflow) and the bytes up to the next 0x7E are dropped.  A closed frame is
 * unescaped (0x7D takes the next byte OR 0x20), an empty one is padding, one whose fcs16 is not 0xF0B8 or whose first byte is not 0x21 is
 * dropped; what remains between the protocol byte and the FCS is one AAS packet: port (16 bits, little endian), seq (the same), data.
 * Deviations: a frame whose last raw byte is an unpaired 0x7D is dropped ("truncated escape"; the reference ORs one stale byte of its
 * buffer in, and the FCS then fails); a packet shorter than port + seq is dropped as wrong protocol (the reference reads past it). */
typedef struct nrsc5hip_psd nrsc5hip_psd;
/* data / len: what follows port and seq */
typedef void (*nrsc5hip_aas_cb)(void *opaque, int stream, unsigned program, unsigned port, unsigned seq, const uint8_t *data, unsigned len);
/* nstreams consumer streams on the engine's device; destroy the consumer before its engine */
int nrsc5hip_psd_create(nrsc5hip_engine *e, int nstreams, nrsc5hip_psd **out);
void nrsc5hip_psd_destroy(nrsc5hip_psd *p);
int nrsc5hip_psd_reset(nrsc5hip_psd *p, int stream);                 /* all eight indices to -1 (frame_reset, frame.c:730-733) */
/* The contract of nrsc5hip_hdc_feed: the same records, lists and targets, the frames must still be in the ring slots the records name,
 * and ids out of range (engine or consumer), a NULL records[i] with counts[i] > 0, a mode that is neither FM nor AM and a record that
 * names a slot the engine does not have are NRSC5HIP_EINVAL before anything is touched; so is a consumer stream listed twice.  A record
 * with NRSC5HIP_REC_TO_FINE closes the stream's eight programs before that record's frames (sync.c:405-409); a loss of sync changes
 * nothing.  ONE index launch, ONE k_psd launch (a wave64 workgroup per listed stream) and one copy of the finished packets for the whole
 * call.  Packets are delivered through cb (may be NULL: count only) inside the call, all of stream_ids[0] first, each stream's in the
 * order of its bytes; `program` is the program whose PDU carried the closing flag.  Returns the number of packets or a negative error; a
 * session may be fed in any number of calls.
 * Frames whose PCI announces fixed-data sub-channels (NRSC5HIP_L2_PCI_HAS_FIXED, and the fixed-only PCI): their index and PDU bytes --
 * only theirs -- are copied to the host, where process_fixed_data's state (private to the consumer, cleared on NRSC5HIP_REC_TO_FINE like
 * nrsc5hip_hdc_frame_reset) gives the cut (nrsc5hip_hdc_fixed_audio_end, nrsc5hip_l2_apply_audio_end).  A header expansion running into
 * the fixed region is NRSC5HIP_EINVAL as in nrsc5hip_hdc_feed: the PSD states are untouched then, the fixed-data state has advanced.
 * With several streams in the call, the fixed-data states of the streams listed in front of the failing frame have advanced over their
 * whole record lists, the failing stream's up to that frame.  Each fixed-data frame costs two blocking copies of its own (index struct,
 * PDU bytes: about 21 KB for a P1 frame), issued frame by frame between the two launches; no byte bound holds for such sessions.
 * Device -> host per call otherwise: 4 bytes per frame of the call (the PCI words, one strided copy), 16 bytes of arena header, and per
 * packet 12 bytes + its data padded to 4 -- so "the packets + 16 bytes each + 256 bytes per listed stream" holds up to 60 frames per
 * stream and call, and the frames themselves never cross.
 * NRSC5HIP_EOVERFLOW: the packet arena, sized from the host-known bounds, was too small (never a silent drop). */
int nrsc5hip_psd_feed(nrsc5hip_psd *p, nrsc5hip_engine *e, int nstreams, const int *stream_ids, const int *targets,
                      const nrsc5hip_record *const *records, const int *counts, int mode, nrsc5hip_aas_cb cb, void *opaque);
/* Counters of one consumer stream since its creation: [0] PDUs walked, [1] span bytes, [2] frames closed, [3] empty frames, [4] bad FCS,
 * [5] wrong protocol, [6] truncated escape, [7] overflows, [8] packets delivered ([2] = [3] + ... + [6] + [8]); [9] bytes the feeds copied
 * device -> host, total over the consumer. */
int nrsc5hip_psd_stats(nrsc5hip_psd *p, int stream, long long stats[10]);
/* stage-level twin: nframes logical frames given as frame_push takes them (one bit per byte, nbits each; as nrsc5hip_stage_l2_index), of
 * logical channel lc, fed in order to consumer stream `stream` through the production index kernel and k_psd */
int nrsc5hip_stage_psd(nrsc5hip_psd *p, nrsc5hip_engine *e, int stream, const uint8_t *bits, int nbits, int nframes, int lc,
                       nrsc5hip_aas_cb cb, void *opaque);
/* ... and the same for several consumer streams in ONE call, the shape of a feed: one index launch over all frames, one k_psd launch with a
 * workgroup per listed stream, one arena, delivery "all of targets[0] first".  Stream i of the call: consumer stream targets[i] (no stream
 * twice), nframes[i] frames of nbits[i] bits at bits[i], logical channel lcs[i].  reset_at (may be NULL; entries < 0: none): the stream
 * gets what a NRSC5HIP_REC_TO_FINE record does -- its eight programs closed, the fixed-data state cleared -- in front of frame reset_at[i],
 * or behind the last frame when reset_at[i] == nframes[i] (a record that announces no frame). */
int nrsc5hip_stage_psd_streams(nrsc5hip_psd *p, nrsc5hip_engine *e, int nstreams, const int *targets, const uint8_t *const *bits,
                               const int *nbits, const int *nframes, const int *lcs, const int *reset_at, nrsc5hip_aas_cb cb, void *opaque);

/* ---- SIS: station id, names, slogan, message, location, service descriptors, alerts (device side: csrc/k_sis.hip) -------------
 * Every block record carries its 80-bit PIDS frame; the reference turns these frames into station information in pids_frame_push ->
 * sis_decode (pids.c).  This consumer does that on the device: per consumer stream it keeps pids_t (pids.h:41-96, 1.4 KB) in device
 * memory, one k_sis launch serves a whole feed (a wave64 workgroup per listed stream: CRC-12, payload walk and field extraction one lane
 * per frame, then the extracted fields applied to the state frame by frame), and only events are copied back: one per state change the
 * reference reports through nrsc5_report_station_id / _name / _slogan / _message / _location / _asd / _dsd / _emergency_alert /
 * _leap_second_offset / _local_time / _exciter_info / _importer_info, in the reference's callback order.  The aggregated, deprecated
 * NRSC5_EVENT_SIS is not an event: it is the snapshot nrsc5hip_sis_get returns.
 * Text is delivered raw with its encoding (0: ISO-8859-1, 4: UCS-2, anything else: the reference reports a NULL string), cut at the first
 * NUL where the reference uses strlen (short name, universal short name, long name); latitude and longitude are the signed 22-bit
 * integers, degrees * 8192.  Alerts carry the control bytes and the text bytes; categories and location lists are not decoded.
 * Deviations: where the reference's completeness loops run past one of its have_frame arrays -- message_len >= 191, slogan_len >= 96,
 * alert_len >= 382, lengths no set of frames can carry -- the item is never complete and a counter says so.  A frame 0 with the same seq may rewrite
 * the length of an item that is displayed (the reference's report() then reads past its arrays): the snapshot shows at most the 190 / 95 / 381 bytes
 * the buffers hold, and the control data within the alert. */
enum {
    NRSC5HIP_SIS_STATION_ID = 1,       /* v[0] facility id; data: the two country-code characters */
    NRSC5HIP_SIS_STATION_NAME,         /* data: the name ("-FM" appended where the frames say so), enc */
    NRSC5HIP_SIS_STATION_SLOGAN,       /* data: the slogan, or the long name (enc 0) */
    NRSC5HIP_SIS_STATION_MESSAGE,      /* v[0] priority; data, enc */
    NRSC5HIP_SIS_STATION_LOCATION,     /* v[0] latitude * 8192, v[1] longitude * 8192, v[2] altitude */
    NRSC5HIP_SIS_AUDIO_SERVICE,        /* v[0] program, v[1] access, v[2] type, v[3] sound_exp */
    NRSC5HIP_SIS_DATA_SERVICE,         /* v[0] access, v[1] type, v[2] mime_type */
    NRSC5HIP_SIS_ALERT,                /* v[0] control data length, data: control bytes then text bytes, enc; v[0] = -1, no data: the alert timed out */
    NRSC5HIP_SIS_LEAP_SECOND,          /* v[0] pending offset, v[1] current offset, v[2] pending ALFN (unsigned) */
    NRSC5HIP_SIS_LOCAL_TIME,           /* v[0] UTC offset in minutes, v[1] dst_regional, v[2] dst_local, v[3] dst_schedule */
    NRSC5HIP_SIS_EXCITER,              /* v[0..3] parameters 4..7 as transmitted (pids.c:698-719 says what they hold) */
    NRSC5HIP_SIS_IMPORTER              /* v[0..3] parameters 8..11 (pids.c:725-744) */
};
#define NRSC5HIP_SIS_NSTATS 31
typedef struct nrsc5hip_sis nrsc5hip_sis;
/* frame: index of the firing frame in the stream's list of this call (records with NRSC5HIP_REC_PIDS, in order; stage hook: frames) */
typedef void (*nrsc5hip_sis_cb)(void *opaque, int stream, int frame, int kind, const int32_t v[8], int enc, const uint8_t *data, unsigned len);
/* what report() (pids.c:284-383) would pass: lengths < 0 mean "none" */
typedef struct nrsc5hip_sis_info {
    char country_code[4]; int32_t fcc_facility_id;                       /* "" and -1: none yet */
    int32_t name_enc, name_len; uint8_t name[16];
    int32_t slogan_enc, slogan_len; uint8_t slogan[96];
    int32_t message_enc, message_len; uint8_t message[192];
    int32_t alert_enc, alert_len, alert_cnt_len; uint8_t alert[384];    /* control bytes [0, alert_cnt_len), then the text */
    int32_t have_location, latitude, longitude, altitude;
    int32_t n_audio, audio[8][4];                                        /* program, access, type, sound_exp */
    int32_t n_data, data[16][3];                                         /* access, type, mime_type */
} nrsc5hip_sis_info;
/* nstreams consumer streams on the engine's device; destroy the consumer before its engine */
int nrsc5hip_sis_create(nrsc5hip_engine *e, int nstreams, nrsc5hip_sis **out);
void nrsc5hip_sis_destroy(nrsc5hip_sis *s);
int nrsc5hip_sis_reset(nrsc5hip_sis *s, int stream);                     /* the state pids_init leaves */
/* records[i][0 .. counts[i]) of consumer stream targets[i] (NULL: stream i), FM or AM records alike: every record with NRSC5HIP_REC_PIDS
 * gives one frame, a record with NRSC5HIP_REC_TO_FINE resets the stream's state in front of its frame (decode_reset, sync.c:407).  16 bytes
 * per record go up, ONE k_sis launch runs, the arena header and the events come back.  Events are delivered through cb (may be NULL: count
 * only) inside the call, all of targets[0] first, each stream's in frame order and within a frame in the reference's callback order.
 * Returns the number of events or a negative error.  A target out of range, a stream listed twice and NULL records with a count > 0 are
 * NRSC5HIP_EINVAL and leave everything untouched.  NRSC5HIP_EOVERFLOW: the event arena, sized from host-known bounds, was too small
 * (never a silent drop); the states have advanced, the events of the call are lost. */
int nrsc5hip_sis_feed(nrsc5hip_sis *s, int nstreams, const int *targets, const nrsc5hip_record *const *records, const int *counts,
                      nrsc5hip_sis_cb cb, void *opaque);
int nrsc5hip_sis_get(nrsc5hip_sis *s, int stream, nrsc5hip_sis_info *out);
/* Counters of one consumer stream since its creation: [0] frames, [1] CRC-12 good, [2] SIS type, [3] LLDS type, [4 + id] payloads decoded by
 * message id (0..15), [20] walks ended by an unknown id (11..15), [21] by a payload with no room, [22] [23] [24] never-complete attempts
 * (message, slogan, alert), [25] bad message checksum, [26] bad alert crc7, [27] bad alert control-data length, [28] bad control-data
 * CRC, [29] events; [30] bytes the feeds copied device -> host, total over the consumer. */
int nrsc5hip_sis_stats(nrsc5hip_sis *s, int stream, long long stats[NRSC5HIP_SIS_NSTATS]);
/* stage hook, through the production kernel: frames[i] = nframes[i] frames of 80 bits, one per byte, exactly as handed to pids_frame_push,
 * for consumer stream targets[i]; reset_at as in nrsc5hip_stage_psd_streams (NULL / < 0: none; == nframes[i]: behind the last frame) */
int nrsc5hip_stage_sis(nrsc5hip_sis *s, int nstreams, const int *targets, const uint8_t *const *frames, const int *nframes,
                       const int *reset_at, nrsc5hip_sis_cb cb, void *opaque);
/* TEST HOOK, not for callers (tests/sis_checks.py provokes NRSC5HIP_EOVERFLOW with it): the event arena of the following calls holds at most
 * `bytes` (0: sized from the host-known bounds again) */
int nrsc5hip_sis_debug_arena(nrsc5hip_sis *s, long long bytes);

/* ---- Data services: the Station Information Guide and LOT files -- album art, station logos (device side: csrc/k_aas.hip) ------
 * The AAS packets the PSD transport reassembles go, in the reference, to output_aas_push (output.c:874-896).  This consumer is chained
 * behind the PSD consumer: k_aas reads the packet arena k_psd leaves in device memory, and only events are copied to the host.  Per
 * consumer stream it keeps, in device memory, the SIG table (16 services x 8 components and the service names, 5.8 KB), lot_lru_counter
 * and `lot_files` file slots (a descriptor of 336 bytes and 65 536 data bytes each).
 * Routing (output.c:874-896): port 0x5100 / 0x5201..0x5207 -> a PSD event: the packet untouched (program, port, seq, data), for the ID3
 * parser; port 0x20 -> SIG; ports 0x0401..0x50FF -> process_port; any other port is counted ([7]).
 * SIG (parse_sig, output.c:512-625): processed while services[0] is empty, i.e. once per stream unless it yields no service.  Element
 * 0x4x opens a service (audio iff the byte is 0x40; number: 16 bits; 3 bytes skipped; a number already in the table clears and reuses that
 * slot, output.c:540-546; a 17th service ends the parse, :549-553).  Element 0x6x: a length byte l, then the value; 0x69 the name, l - 2
 * bytes from p + 1 (:571-574); 0x67 a data component (id, port, service_data_type, type, mime at p + 8; :575-594); 0x66 an audio component
 * (id, port, type, mime at p + 7; :595-613); an id already in the service overwrites its slot, a 9th component ends the parse
 * (find_component, :493-510); a 0x6x in front of any service ends the parse (:566-570); p += l - 1 (:614).  Any other byte ends the parse
 * (:617-619).  The SIG event is emitted at the end of the parse in every case (:623-624).
 *   Deviations, each counted: every read is checked against the packet, and an element whose bytes (service number; length byte; name with
 *   l < 2 or running past the packet; the 12 / 11 bytes of a component) do not lie inside it ends the parse ([4]); so does l == 0 ([5]).  The
 *   reference reads past the packet, or walks backwards.  A SIG that yields no service emits an event with an empty table ([6]); the
 *   reference hands out an uninitialised pointer.  A name of length 0 is reported as no name (the reference reports an empty string).
 * process_port (output.c:684-872): a packet in front of the SIG is dropped ([8], :688-692); the port is looked up as the first data
 * component with that port, in service order (find_port, :627-647); not found: counted ([9]).  Type 0: a STREAM event, type 1: a PACKET
 * event (port, seq, mime, data; :703-714); type 3: LOT; any other type is counted ([12]).  HERE-image assembly (here_images.c) is not done:
 * its stream packets are STREAM events like any other.
 * LOT (output.c:715-866), in the reference's order: the packet is dropped ([14]) if len < 8 (:717), if hdrlen < 8 or hdrlen > len (:726), or
 * if seq >= 256 (:735).  find_lot matches the lot among the component's live files (:649-659); otherwise find_free_lot takes the
 * component's first free file or its least recently used of 12, the first of equals (:661-682).  The timestamp is taken from the counter
 * before the header is looked at (:748), so a packet with 0 < hdrlen - 8 < 16 returns with the file allocated and stamped ([15], :754-758).
 * Header: version, expiry (year - 1900, mon - 1, mday, hour, min from bytes 4..7, :764-768), size, mime; the name is the rest of the header,
 * kept cut at its first NUL, and compared as "length sent != length kept, or the bytes differ" (strlen on the strndup copy, :779-780, 804).
 * Changed metadata resets the file: its timestamp becomes the counter's current value and new_data is set ([17], :788-795).  LOT_HEADER is
 * emitted iff the header set new_data (:817-822).  A new fragment with len > 256 leaves the packet without a store or an event ([20],
 * :831-835); otherwise len bytes are stored at seq * 256, the remaining 256 - len zeroed, and len added to bytes_so_far (:830-838).  A
 * LOT_FRAGMENT event follows for new and duplicate fragments alike (:840).  The completeness test runs iff new_data && size, over
 * fragments 0 .. ceil(size / 256) - 1 (:843-854); the LOT event carries lot, size, mime, name, expiry and the first `size` bytes.
 *   Deviations: size > 65 536 can never complete ([22]; the reference runs past its fragment array).  LOT_FRAGMENT events never carry the
 *   fragment's bytes, and are written only with NRSC5HIP_AAS_FRAGMENTS; [18] and [19] count them in either case.  A component never
 *   holds more than 12 live files, as in the reference ([23] counts its evictions); the slots behind them are a pool of `lot_files` per stream,
 *   and when all are in use and a file is needed the stream's least recently stamped file is evicted (the lowest slot of equals) and [24] counts
 *   it -- this can only happen when more files are live than the pool has slots, and never silently.
 * Events, in the arena and through the callback: kind, port, seq, v[8], data --
 *   PSD           port, seq, v[0] program; data: what follows port and seq
 *   SIG           v[0] services; data, per service: type (1 data, 2 audio), number (16 bits, little endian), name length, the name (raw
 *                 ISO-8859-1: the reference converts it to UTF-8), component count; per component: type (1 data, 2 audio), id, port (16 bits),
 *                 service_data_type (16 bits), type, mime (32 bits) -- 11 bytes; an audio component has service_data_type 0
 *   LOT_HEADER    port, v[0] lot, v[1] size, v[2] mime, v[3..7] tm_year, tm_mon, tm_mday, tm_hour, tm_min; data: the name
 *   LOT_FRAGMENT  port, seq, v[0] lot, v[1] repeat, v[2] is_duplicate, v[3] size, v[4] bytes_so_far; no data
 *   LOT           as LOT_HEADER, seq = the length of the name; data: the first `size` bytes of the file, then the name
 *   STREAM / PACKET   port, seq, v[0] mime, v[1] service, v[2] component (indices into the table); data
 * An event takes 48 bytes and its data, padded to 4, in the arena. */
enum { NRSC5HIP_AAS_PSD = 1, NRSC5HIP_AAS_SIG, NRSC5HIP_AAS_LOT_HEADER, NRSC5HIP_AAS_LOT_FRAGMENT, NRSC5HIP_AAS_LOT, NRSC5HIP_AAS_STREAM, NRSC5HIP_AAS_PACKET };
#define NRSC5HIP_AAS_FRAGMENTS 1       /* flags of nrsc5hip_aas_create: write LOT_FRAGMENT events */
#define NRSC5HIP_AAS_NSTATS 27
#define NRSC5HIP_AAS_SIG_MAX 5632      /* bytes a SIG table can take in the layout above: 16 x (5 + 253 + 8 x 11) */
typedef struct nrsc5hip_aas nrsc5hip_aas;
typedef void (*nrsc5hip_aas_event_cb)(void *opaque, int stream, int kind, unsigned port, unsigned seq, const int32_t v[8], const uint8_t *data, unsigned len);
/* nstreams consumer streams on the engine's device, lot_files (1..64) file slots each; destroy the consumer before its engine */
int nrsc5hip_aas_create(nrsc5hip_engine *e, int nstreams, int lot_files, int flags, nrsc5hip_aas **out);
void nrsc5hip_aas_destroy(nrsc5hip_aas *a);
int nrsc5hip_aas_reset(nrsc5hip_aas *a, int stream);                  /* aas_reset, output.c:182-202: table and files gone, the counter 1 */
/* nrsc5hip_psd_feed with the data services chained behind it: the same records, lists, targets and rejections (a target must lie inside
 * both consumers), the fixed-data cut on the host as there, and `psd` advances exactly as nrsc5hip_psd_feed would advance it -- but its
 * packet arena is not copied back: ONE k_aas launch (a wave64 workgroup per listed stream) runs over it, and the header and the used part
 * of the event arena come back.  Events are delivered through cb (may be NULL: count only) inside the call, all of stream_ids[0] first,
 * each stream's in packet order and those of one packet in the reference's callback order: LOT_HEADER, LOT_FRAGMENT, LOT.  Returns the
 * number of events or a negative error.  A NRSC5HIP_REC_TO_FINE record resets HDLC state only: the data-service state survives a resync,
 * as output_t does in the reference.
 * Device -> host per call: what nrsc5hip_psd_feed moves without its arena (4 bytes per frame; fixed-data frames as there), 16 bytes of
 * arena header, and per event 48 bytes + its data padded to 4.  The bytes of a LOT fragment cross only inside a complete file.
 * The event arena is sized from what the host knows: four times the packet arena (an event is at most four times its packet's record,
 * whatever the packet turns into except a complete file or the SIG), and per listed stream 8 KB for the SIG and lot_files x (65 536 + 512)
 * for complete files: every file slot may complete once per call.  NRSC5HIP_EOVERFLOW: the event arena, or the packet arena in front of
 * it, was too small (never a silent drop); the states have advanced, the events of the call are lost. */
int nrsc5hip_aas_feed(nrsc5hip_aas *a, nrsc5hip_psd *psd, nrsc5hip_engine *e, int nstreams, const int *stream_ids, const int *targets,
                      const nrsc5hip_record *const *records, const int *counts, int mode, nrsc5hip_aas_event_cb cb, void *opaque);
/* Counters of one consumer stream since its creation: [0] packets, [1] PSD-port packets passed on, [2] SIG packets, [3] SIGs parsed,
 * [4] parses ended by a truncated element, [5] by l == 0, [6] SIGs without a service, [7] unknown port range, [8] packets in front of the
 * SIG, [9] port not in the table, [10] STREAM, [11] PACKET events, [12] unknown component type, [13] LOT packets, [14] dropped (len,
 * hdrlen, seq), [15] header too short, [16] LOT_HEADER events, [17] files reset by changed metadata, [18] fragments (new and duplicate),
 * [19] duplicates, [20] fragments over 256 bytes, [21] LOT events, [22] completeness tests of a size over 65 536, [23] evictions by the
 * component's LRU, [24] by the pool, [25] events written; [26] bytes the feeds copied device -> host, total over the consumer (the PSD
 * consumer in front counts its own). */
int nrsc5hip_aas_stats(nrsc5hip_aas *a, int stream, long long stats[NRSC5HIP_AAS_NSTATS]);
/* the stream's SIG table as a snapshot, in the layout of the SIG event's data (what that event held), for callers that joined late:
 * out[NRSC5HIP_AAS_SIG_MAX], *len its bytes, *nservices 0 while no SIG has been seen */
int nrsc5hip_aas_sig(nrsc5hip_aas *a, int stream, uint8_t *out, unsigned *len, int *nservices);
/* stage hook, through the production kernel: AAS packets per consumer stream targets[i] (NULL: stream i) -- packets[i]: nbytes[i] bytes,
 * packet after packet, each as four little-endian 16-bit words (port, seq, data length, program) and then its data -- uploaded as one
 * PsdPacket arena, the streams interleaved packet by packet */
int nrsc5hip_stage_aas(nrsc5hip_aas *a, int nstreams, const int *targets, const uint8_t *const *packets, const int *nbytes,
                       nrsc5hip_aas_event_cb cb, void *opaque);
/* stage hook of the chain, frames -> index -> k_psd -> k_aas: the arguments of nrsc5hip_stage_psd_streams */
int nrsc5hip_stage_aas_frames(nrsc5hip_aas *a, nrsc5hip_psd *psd, nrsc5hip_engine *e, int nstreams, const int *targets, const uint8_t *const *bits,
                              const int *nbits, const int *nframes, const int *lcs, const int *reset_at, nrsc5hip_aas_event_cb cb, void *opaque);
/* TEST HOOK, not for callers: as nrsc5hip_sis_debug_arena, for the event arena */
int nrsc5hip_aas_debug_arena(nrsc5hip_aas *a, long long bytes);

/* ---- stage-level entry points (host buffers): parity tests of single kernels against the oracle ---- */
int nrsc5hip_stage_halfband_fm_cu8(nrsc5hip_engine *e, const uint8_t *iq, uint32_t nbytes, int16_t *out /* [nbytes/4][2] */);
int nrsc5hip_stage_fft2048(nrsc5hip_engine *e, const float *in /* [n][2048][2] */, float *out, int n);
int nrsc5hip_stage_viterbi_k7(nrsc5hip_engine *e, const int8_t *soft /* [nframes][3*len] */, int len, int nframes,
                              uint8_t *bits /* [nframes][len] */);
/* K=9 codes of the AM path (nrsc5_conv_decode_e1 / _e2_e3, conv_dec.c:469-478): gens = {0561,0657,0711} or {0561,0753,0711} */
/* frame_process's first-header check (frame.c:516-540: RS(255,247) over the first 96 PDU bytes unless the PCI says "no audio") as the
 * decode kernels run it on a finished P1 frame: `bits` = nframes descrambled frames of nbits (146176 FM / 3750 AM) bits, one per byte;
 * `threads` = workgroup size (64 ... 1024); ok[f] = 1 when the reference would keep the receiver synchronised */
int nrsc5hip_stage_first_header(nrsc5hip_engine *e, const uint8_t *bits, int nbits, int nframes, int threads, int *ok);
int nrsc5hip_stage_viterbi_k9(nrsc5hip_engine *e, const int8_t *soft /* [nframes][3*len] */, int len, int nframes,
                              const unsigned gens[3], uint8_t *bits /* [nframes][len] */);
/* device check of the DPP / v_permlane / v_writelane / v_dot4 helpers against generic shuffles: *failures == 0 */
int nrsc5hip_stage_selftest(nrsc5hip_engine *e, int *failures);
/* The device's math header (csrc/fastmath.h) on caller data, one work-item per element: what the parity contract rests on (ref_sincosf /
 * ref_atan2f = glibc's sincosf / atan2f bit for bit) and the short forms of the sync chain, evaluated by the gfx950 code itself.  n
 * elements; a, b, out0, out1 are HOST arrays of float (double for the two series); b and out1 may be NULL where the table says "-":
 *   fn                                 a          b    out0    out1
 *   NRSC5HIP_MATH_REF_SINCOSF          y          -    sin     cos
 *   NRSC5HIP_MATH_REF_ATAN2F           y          x    angle   -
 *   NRSC5HIP_MATH_FAST_SINCOS          x          -    sin     cos
 *   NRSC5HIP_MATH_FAST_SINCOS_REDUCED  x          -    sin     cos       (|x| within a few turns)
 *   NRSC5HIP_MATH_FAST_ATAN2           y          x    angle   -
 *   NRSC5HIP_MATH_SMALL_COS_SIN        x (double) -    cos     sin       (|x| <= 0.25)
 *   NRSC5HIP_MATH_SMALL_ATAN           t (double) -    atan    -         (|t| <= 0.26) */
enum { NRSC5HIP_MATH_REF_SINCOSF = 0, NRSC5HIP_MATH_REF_ATAN2F, NRSC5HIP_MATH_FAST_SINCOS, NRSC5HIP_MATH_FAST_SINCOS_REDUCED,
       NRSC5HIP_MATH_FAST_ATAN2, NRSC5HIP_MATH_SMALL_COS_SIN, NRSC5HIP_MATH_SMALL_ATAN };
int nrsc5hip_stage_math(nrsc5hip_engine *e, int fn, const void *a, const void *b, long long n, void *out0, void *out1);
/* The float32 half-band of the zero-copy batch (csrc/halfband_raw.h) on caller data, evaluated by the production functions themselves in
 * one of the three forms the device runs it in:
 *   NRSC5HIP_HB_ACQ     hb_sample_q15                            one work-item per sample, 256 per workgroup   (k_acq_decimate)
 *   NRSC5HIP_HB_SYM128  raw_symbol_load + raw_symbol_halfband    128 work-items x 17 outputs, one per symbol   (k_mixfft<..>)
 *   NRSC5HIP_HB_SYM256  raw_symbol_load8 + raw_symbol_halfband8  256 work-items x 9 outputs, one per symbol    (k_mixfft8)
 * iq: nbytes HOST bytes of a cu8 capture (stream start at byte 0; zero history in front of it), placed `lead` (0, 4, 8 or 12) bytes into
 * a 16-byte-aligned device buffer.  a0: the first decimated sample; n: the number of SYMBOLS of 2160 samples (symbol forms) or of
 * samples (NRSC5HIP_HB_ACQ).  out[.][2]: the Q15 integers of the reference's decimator (firdecim_q15.c), samples a0 .. -- the symbol
 * forms' tile holds the imaginary part negated, the kernel turns it back.  probe (NULL: none; symbol forms only): per symbol and
 * work-item four words -- the bits of 1.0f + 1.5 * 2^-24 and of 2^-126 * 0.5f, operands read from memory, evaluated before the half-band
 * and again behind it: 0x3f800001 and 0x00200000 in round-to-nearest with denormals kept (0x3f800000 when rounding down).
 * NRSC5HIP_EINVAL, nothing launched: unknown form; lead not in {0, 4, 8, 12}; n < 1; a0 < 0; nbytes % 4 != 0; a request whose last output
 * needs a raw sample beyond nbytes (4 (a0 + outputs) > nbytes).  Nothing outside the uploaded bytes is read. */
enum { NRSC5HIP_HB_ACQ = 0, NRSC5HIP_HB_SYM128, NRSC5HIP_HB_SYM256 };
int nrsc5hip_stage_halfband_raw(nrsc5hip_engine *e, int form, const uint8_t *iq, size_t nbytes, int lead, long long a0, long long n,
                                int16_t *out, uint32_t *probe);
/* ---- the FEC stage's permutations, error counts and descramblers on caller data (tests/fec_checks.py) ----------------------------------
 * Each hook runs the PRODUCTION device code -- the production kernels themselves on stream 0 of the engine, which must exist and is left
 * freshly reset (as nrsc5hip_stage_halfband_fm_cu8 does), or the production __device__ function called by a small stage kernel -- and
 * returns what it wrote, raw.  NRSC5HIP_EINVAL with nothing launched: a null pointer, an unsupported length, a count below 1, an unknown
 * mode / code / workgroup size.
 * p1_deint: k_p1_deint (interleaver I + depuncture through tb.deint_lut).  pm int8 [16][23040], one L1 frame's soft-bit matrices ->
 *   out [146176] dwords, one per trellis step: s0 | s1 << 8 | s2 << 16, punctured positions 0, byte 3 zero. */
int nrsc5hip_stage_p1_deint(nrsc5hip_engine *e, const int8_t *pm, uint32_t *out);
/* p1_frame: k_p1_forward + k_p1_fix + the traceback of the form `walk` selects (the value of NRSC5HIP_TUNE_TRACEBACK_WALK, 0 or 1; with
 *   1 the re-encode count is the per-chunk counts of k_p1_tbwalk plus the six wrapped bits, with 0 the one loop of k_p1_traceback), l2_mode 0,
 *   NRSC5HIP_TUNE_FWD_SEGMENTS honoured (16 when it is 0).  soft int8 [3 * 146176] as nrsc5hip_stage_viterbi_k7 takes it -> bits [146176]
 *   after the descramble, *errors = the integer the BER record is made of. */
int nrsc5hip_stage_p1_frame(nrsc5hip_engine *e, const int8_t *soft, int walk, uint8_t *bits, int *errors);
/* pids: the gather + depuncture of block bc (0..15) through tb.pids_gather, then k_pids_decode (pids_decode_wave: 80-bit trellis, descramble,
 *   CRC-12).  pm int8 [16][23040] -> coded [240], bits [80], *crc_ok. */
int nrsc5hip_stage_pids(nrsc5hip_engine *e, const int8_t *pm, int bc, int8_t *coded, uint8_t *bits, int *crc_ok);
/* px_interleave: k_px_deint + k_px_commit (interleaver IV through tb.px_delay_*) once per block pair, both channels live, from a fresh
 *   interleaver state.  len 2304 or 4608; pairs int8 [npairs][2 channels][2 * len] -> out int8 [npairs][2][3 * len] (depunctured), ready[npairs]. */
int nrsc5hip_stage_px_interleave(nrsc5hip_engine *e, int len, int npairs, const int8_t *pairs, int8_t *out, int *ready);
/* am_deinterleave (engine with am_enable): k_am_interleave, all its slices and the commit, once per L1 frame from a fresh 3-frame delay ring.
 *   psmi 1 (MA1) or 2 (MA3); sym uint8 [nframes][4][6400] in the order pl, pu, s, t -> v1 int8 [nframes][90000], v3 int8 [nframes][72000 (MA1) or 90000]. */
int nrsc5hip_stage_am_deinterleave(nrsc5hip_engine *e, int psmi, int nframes, const uint8_t *sym, int8_t *v1, int8_t *v3);
/* am_epilogue: am_bit_errors + am_descramble (k_am_decode.hip: am_p3_epilogue over am_decode_frame's choice of code) by one workgroup of
 *   `threads` (64 or 256) work-items.  (len, code): (3750, NRSC5HIP_CODE_E1), (24000, NRSC5HIP_CODE_E2), (30000, NRSC5HIP_CODE_E1); soft int8 [3 * len],
 *   bits uint8 [len] (the decoded, still scrambled frame -- the caller's choice) -> *errors, bits_out [len] and words_out [(len + 31) / 32] after the descramble. */
enum { NRSC5HIP_CODE_E1 = 1, NRSC5HIP_CODE_E2 = 2 };
int nrsc5hip_stage_am_epilogue(nrsc5hip_engine *e, const int8_t *soft, const uint8_t *bits, int len, int code, int threads, int *errors,
                               uint8_t *bits_out, uint32_t *words_out);
/* ---- coarse acquisition on caller data (ABI 13; tests/acq_checks.py) ------------------------------------------------------------------
 * Each hook runs the PRODUCTION launch -- launch_acquire (k_acq_list, k_acq_decimate, k_acq_fir, k_acq_corr, k_acq_peak) on streams 0 .. n-1 of the
 * engine, or launch_am_step (k_am_block, whose first section is the AM acquisition) on stream 0 -- once, on freshly reset streams into which it
 * wrote the caller's window, the acquisition filter's 31-sample history and the sync state, and returns what the kernels left, raw.  Everything
 * they may write is filled with 0xA5 bytes first (int16 -23131, the float with the bits 0xA5A5A5A5, samperr 0xA5A5A5A5): a stream the
 * acquisition must skip -- one that is FINE, or short of a window -- still shows the fill, and its history is what went in.  The streams are left
 * freshly reset.  state: 0 NONE, 1 COARSE, 2 FINE.  All arrays are HOST arrays, [n] leading; c16 samples as int16 [.][2].
 * NRSC5HIP_EINVAL with nothing launched: a null pointer; n < 1 or n > max_streams; q15_capacity below a window; a state outside the three; a
 * stream in the other mode; a fill outside 0 .. window; (am_acquire) an engine without am_enable; (acquire_raw) an engine without
 * batch_zero_copy, nbytes % 4 != 0, rd < 0 or 4 * (rd + 71280) > nbytes.
 * acquire: the FIFO seam.  win [n][71280][2] goes to the start of each stream's FIFO slab, fill[n] (<= 71280) is its write position: below 71280
 *   the stream has no complete window.  -> filt [n][71280][2] (acq_filt), sums float [n][2160][2] (acq_sums), samperr [n], peak float [n][2]
 *   (coarse_samperr, coarse_re / coarse_im), hist_out [n][31][2] (fir_hist afterwards). */
int nrsc5hip_stage_acquire(nrsc5hip_engine *e, int n, const int16_t *win, const int16_t *hist, const int *state, const int *fill,
                           int16_t *filt, float *sums, int *samperr, float *peak, int16_t *hist_out);
/* acquire_raw: the zero-copy seam (engine with batch_zero_copy).  iq [n][nbytes]: cu8 captures, uploaded and attached the way
 *   nrsc5hip_batch_append_cu8 attaches them (stride nbytes); rd[n]: the read position, in decimated samples, the window starts at -- k_acq_decimate
 *   produces it.  Additionally -> acq_win [n][71280][2], the decimated window. */
int nrsc5hip_stage_acquire_raw(nrsc5hip_engine *e, int n, const uint8_t *iq, long long nbytes, const long long *rd, const int16_t *hist, const int *state,
                               int16_t *acq_win, int16_t *filt, float *sums, int *samperr, float *peak, int16_t *hist_out);
/* am_acquire: stream 0 of an am_enable engine, in AM mode.  win [8910][2], hist [31][2], fill <= 8910.  One whole block step: k_am_block<256> on an
 *   engine without p1_async, k_am_block<512> (window pipeline: parity 0, slot 0, window 0) on one with it.  The filtered window and the sums live in
 *   LDS and stay unobserved; nothing behind the acquisition section writes coarse_samperr / coarse_re / coarse_im / fir_hist, so they are read from the
 *   stream state after the step: -> *samperr, peak [2], hist_out [31][2]. */
int nrsc5hip_stage_am_acquire(nrsc5hip_engine *e, const int16_t *win, const int16_t *hist, int state, int fill, int *samperr, float *peak, int16_t *hist_out);
/* ---- the AM block step on caller data (ABI 18; tests/am_checks.py) ----------------------------------------------------------------------------
 * Runs k_am_block ALONE -- the first launch of launch_am_step, without the decode and interleave launches behind it -- once on stream 0 of an am_enable
 * engine in AM mode, freshly reset, into whose state the hook wrote the caller's window (win [8910][2], fill <= 8910 = the FIFO's write position), the
 * acquisition filter's history (hist [31][2]) and the state words of *in.  The launch shape follows the engine as in nrsc5hip_stage_am_acquire:
 * k_am_block<256> with pipeline = 0 on an engine without p1_async, k_am_block<512> with pipeline = 1 (window parity 0, slot 0) on one with it.  dump != 0
 * selects the instantiation that also copies the tile out: spectra float [32][256][2] = the 32 symbol spectra behind the sideband combine (FFT order: bin k of
 * the carrier at index k & 255), mult float [4][25][2] = the equaliser taps (pl, pu, s, t; written only by a block that is FINE at its end).  Everything the
 * kernel may write is filled with 0xA5 bytes first: the record, am_sym, the staged PIDS bytes, spectra and mult.  ->  *rec: the block's record (record slot
 * 0); *out: the same state words after the launch, with the read-only ones; am_sym uint8 [4][6400]: the stream's whole hard-symbol matrices; pids_stage
 * int8 [240]: the pipeline form's staged trellis input (in order: still the fill; rec->pids and NRSC5HIP_REC_PIDS_CRC hold the decode).  The stream is left
 * freshly reset.  No arithmetic lives in the hook.  NRSC5HIP_EINVAL with nothing launched: a null pointer (spectra / mult may be null when dump == 0); an
 * engine without am_enable; a stream in FM mode; in->sync_state outside 0 .. 2; in->bc outside 0 .. 7; in->samperr outside -135 .. 135 or in->coarse_samperr
 * outside 0 .. 269 (the window would be read out of range); fill outside 0 .. 8910. */
typedef struct nrsc5hip_am_block_state {
    int32_t sync_state, samperr, cfo, psmi, bc, cfo_wait;      /* StreamState */
    float prev_angle, angle;
    double theta;
    int32_t coarse_samperr; float coarse_re, coarse_im;         /* (overwritten by the acquisition section while not FINE) */
    int32_t keep_extra;
    uint32_t offset_history;                                    /* AmStream */
    int32_t rdbi, pli, hppi, aabi, am_diversity_wait;
    uint32_t am_errors;
    int32_t fine_epoch, active, nblocks;                        /* read back only: ignored in *in */
    long long rd;
} nrsc5hip_am_block_state;
int nrsc5hip_stage_am_block(nrsc5hip_engine *e, const int16_t *win, const int16_t *hist, const nrsc5hip_am_block_state *in, int fill, int dump,
                            nrsc5hip_record *rec, nrsc5hip_am_block_state *out, uint8_t *am_sym, int8_t *pids_stage, float *spectra, float *mult);
/* ---- the exact oscillator on caller data (ABI 17; tests/nco_checks.py) ---------------------------------------------------------------------
 * Runs the PRODUCTION launch (launch_nco_exact: k_nco_exact) once on streams 0 .. n-1 of the engine, freshly reset, into whose state it wrote what the block's
 * bookkeeping leaves for the kernel: start [n][2] = the oscillator in front of the block (acquire_t.phase after the block-start rotation), inc [n][2] = phase_increment,
 * active [n], nco_mode [n] (the block runs on the table: 1).  -> tab float [n][32 * 2160][2]: the streams' table rows, filled with 0xA5 bytes before the launch -- a
 * stream that is not active or not in exact mode still shows the fill -- and end [n][2]: the stream's oscillator state afterwards (for such a stream: start).  All
 * arrays are HOST arrays.  The streams are left freshly reset.  NRSC5HIP_EINVAL with nothing launched: a null pointer; n < 1 or n > max_streams; a stream in AM mode;
 * an engine without the table. */
int nrsc5hip_stage_nco_exact(nrsc5hip_engine *e, int n, const float *start, const float *inc, const int *active, const int *nco_mode, float *tab, float *end);
/* ---- the FM symbol transform on caller data (ABI 20; tests/sym_checks.py) ---------------------------------------------------------------------
 * Runs the PRODUCTION launch (launch_mixfft: k_mixfft<SPW, NPAR> or k_mixfft8 -- timing pick, in-place cu8 half-band, Q15 -> float, oscillator mix, cyclic-prefix
 * fold, FFT-2048, live-bin cut) once, for one block of 32 symbols, on streams 0 .. n-1 of the engine, freshly reset and in FM mode.  form: the mixfft_syms value
 * handed to launch_mixfft -- 1, 2, 4, 8 (symbols per 128-lane workgroup), 16 (two symbols side by side in 256 lanes), 32 (the 256-lane kernel); the engine's own
 * tune knob is neither read nor changed.  ids: null, or a permutation of 0 .. n-1 (the launch's stream list; in[] and out[] stay indexed by STREAM).
 * Samples of stream s (in[s]): either raw != null -- a cu8 capture of raw_bytes bytes read in place: uploaded `lead` (0, 4, 8 or 12) bytes into a 16-byte aligned
 * temporary buffer and attached as the zero-copy batch attaches one (StreamState::raw, base 0, wr = raw_bytes / 4) -- or q15 != null: q15_samples Q15 samples
 * [.][2] written to the start of the stream's FIFO slab.  nco_tab: null, or float [32][2160][2] copied into the stream's row of the oscillator table.
 * params_mode 0: a00 (first decimated sample of symbol 0), dtheta, theta, growth, active, nco_mode are written to the state words a symbol workgroup reads when
 *   local_prepare = 0 (rd = a00, samperr_cur = 0, dtheta, theta, growth, active, nco_mode); one launch with local_prepare = 0; `prepare` is ignored.
 * params_mode 1: the stream is FINE with samperr, cfo, angle, prev_angle, theta, rd, wr as given and has left exact-oscillator mode (nco_exact 0).
 *   prepare 1: launch_mixfft(local_prepare = 1) alone, as the fused streaming seam launches it; only once the bins are back the hook runs launch_prepare, which
 *   commits the same bookkeeping the way the block step behind the kernel would, so that *out can be read.  prepare 0: launch_prepare, then
 *   launch_mixfft(local_prepare = 0).
 * Before the launch the bins of ALL max_streams streams are filled with 0xA5 bytes.  -> bins float [max_streams][32][534][2], and per stream out[s]: what the
 * kernel ran on, read back from the state.  The streams are left freshly reset, the record and counters the bookkeeping touched cleared, the bins zeroed.  No
 * arithmetic lives in the hook.  NRSC5HIP_EINVAL with nothing launched: a null pointer; n < 1 or n > max_streams; a form outside the six; params_mode / prepare
 * outside 0 .. 1; a stream in AM mode; ids that are no permutation; both or neither of raw / q15; lead outside the four; raw_bytes % 4 != 0 or beyond 2^30;
 * q15_samples beyond q15_capacity; a00 < 0; the last symbol's last sample (a00 + 32 * 2160 - 1) beyond the capture or the window; nco_mode 1 without nco_tab, or
 * an engine without the table; (mode 1) rd < 0, wr beyond the samples given, wr - rd < 71280 (no complete window), samperr outside -1080 .. 1080. */
typedef struct nrsc5hip_sym_stream {
    const uint8_t *raw; size_t raw_bytes; int32_t lead, pad0;
    const int16_t *q15; long long q15_samples;
    const float *nco_tab;
    long long a00; double dtheta, theta, growth; int32_t active, nco_mode;     /* mode 0 (theta: both modes) */
    int32_t samperr, cfo; float angle, prev_angle; long long rd, wr;            /* mode 1 */
} nrsc5hip_sym_stream;
typedef struct nrsc5hip_sym_params { long long a00; double dtheta, theta, growth; int32_t active, nco_mode; } nrsc5hip_sym_params;
int nrsc5hip_stage_symbols(nrsc5hip_engine *e, int n, int form, int params_mode, int prepare, const nrsc5hip_sym_stream *in, const int *ids,
                           float *bins, nrsc5hip_sym_params *out);
/* one frame, also returning the len+64 survivor-decision words of the forward pass */
int nrsc5hip_stage_viterbi_k7_debug(nrsc5hip_engine *e, const int8_t *soft, int len, uint8_t *bits, unsigned long long *dec_out);
/* micro-benchmark of the Viterbi kernel on random frames: phases bit0 = forward, bit1 = traceback */
int nrsc5hip_stage_viterbi_bench(nrsc5hip_engine *e, int len, int nframes, int phases, int reps, float *ms_per_launch);
int nrsc5hip_stage_viterbi_k9_bench(nrsc5hip_engine *e, int len, int nframes, int phases, int reps, float *ms_per_launch);
/* Tuning knobs and test hooks (the library reads nothing from the environment).  Call on an idle engine. */
enum {
    NRSC5HIP_TUNE_DECODE_STREAMS = 0,    /* FM window pipeline: HIP streams that decode windows concurrently (1..5; default 1 since round 5, 3 before) */
    NRSC5HIP_TUNE_AM_DECODE_STREAMS,     /* same for the AM window pipeline (default 3) */
    NRSC5HIP_TUNE_VERDICT_LAG,           /* TEST HOOK: the replay takes first-header verdicts this many windows late (0..8): deep speculation */
    NRSC5HIP_TUNE_SYNC_PHASES,           /* 1: k_sync accumulates shader cycles per phase for stream 0 (nrsc5hip_debug_sync_phases) */
    NRSC5HIP_TUNE_FWD_SEGMENTS           /* waves per frame of the K=7 forward trellis pass (1..64; 0 = chosen from the size of the stream set).  Any value
                                            gives the sequential decoder's decisions bit for bit: segments start speculatively and are verified /
                                            repaired (viterbi_v3.h).  Also used by nrsc5hip_stage_viterbi_k7 / _bench. */
    , NRSC5HIP_TUNE_FWD_WARM               /* TEST HOOK: 0 = the segments start cold (no speculative warm-up), so that the speculation fails wherever the
                                            input carries information and every segment takes the repair path; 1 = normal */
    , NRSC5HIP_TUNE_AM_SEGMENTS            /* waves per P3 frame of the K=9 decode in the AM window pipeline (1..8, default 8); forward pass AND traceback
                                            run in segment waves, both verified / repaired: any value gives the sequential decoder's bits.  Also used by
                                            nrsc5hip_stage_viterbi_k9 / _bench (1 = the single-wave form). */
    , NRSC5HIP_TUNE_DECODE_CUS             /* decode streams confined to value / 32 of every XCD's CUs (8, 16, 24; 32 = all, the default) */
    , NRSC5HIP_TUNE_DECODE_PRIORITY        /* 1: decode streams at the lowest queue priority (default 0: all queues equal) */
    , NRSC5HIP_TUNE_AM_WARM                /* TEST HOOK: 0 = no forward warm-up and no traceback run-in (every boundary takes the repair path); 1 = normal */
    , NRSC5HIP_TUNE_MIXFFT_SYMS            /* OFDM symbols per k_mixfft workgroup: 1 (default), 2, 4, 8 -- any value gives identical bins; 16 = two symbols side by side in a
                                             256-lane workgroup (identical bins); 32 = the 256-lane x 8-point kernel k_mixfft8 (bins within float tolerance); 100 .. 140 =
                                             DIAGNOSTIC: the default kernel with (value - 100) KiB of unused dynamic LDS per workgroup (fewer workgroups per CU; the engine
                                             clamps the padding to what the device's per-workgroup LDS limit leaves); anything else = 1 */
    , NRSC5HIP_TUNE_DEFER_WAIT             /* fast streaming seam: 1 (default) = a block step whose FIFO consumption the host can compute in advance stays in
                                             flight when the push returns; 0 = every step is waited for at once (round 3's behaviour) */
    , NRSC5HIP_TUNE_TRACEBACK_WALK         /* > 0: single-path traceback of the K=7 frames (one speculative walk per chunk, verified, re-walked where wrong): 1 (default) = one workgroup per
                                             (frame, part); N > 1 = a persistent grid of N one-wave workgroups (opt-in: measured slower, profiles/r04_traceback_walk.txt);
                                             0: round 3's block-parallel traceback (all 64 candidates per chunk).  Identical output */
    , NRSC5HIP_TUNE_SYNC_LANES             /* work-items per stream of the sync kernel: 256, 768, 0 = chosen from the size of the stream set (default) */
    , NRSC5HIP_TUNE_DIRECT_DECIMATE        /* fast streaming seam, FM cu8: 1 (default) = the decimator reads the pinned staging buffer across PCIe itself (one
                                             launch per chunk); 0 = hipMemcpyAsync into a device buffer, decimator, commit kernel (round 3's chain) */
    , NRSC5HIP_TUNE_EARLY_FLUSH_KB         /* fast streaming seam with the direct decimator: staged KiB at which a chunk is submitted (on the engine's ingest stream,
                                             beside the running block step) before its block is complete; 0 = only at the block's end.  Default 128 */
    , NRSC5HIP_TUNE_SEAM_PREPARE           /* fast streaming seam, FINE stream: 1 (default) = the block's bookkeeping is computed by the symbol kernel for itself and
                                             committed by the sync kernel; 0 = k_prepare as a launch of its own in front of them */
    , NRSC5HIP_TUNE_NCO_EXACT              /* which blocks of a freshly reset FM stream advance the NCO by the reference's own float recurrence (acquire.c:237-252: 69 120
                                             dependent complex multiplications per block, ~0.4 ms of one lane per stream whatever the number of streams) instead of the
                                             closed-form phasor: 0 = none, 1 (default since round 6) = the first block after a reset (the block the CFO search runs on), 2 = every block until the
                                             stream is FINE, 3 = every block (diagnostic).  The float oscillator state is the reference's bit for bit for as long as every
                                             block since the reset ran in this mode; the first closed-form block ends that until the next reset */
    , NRSC5HIP_TUNE_FLOW_MIN               /* dataflow bursts (k_flow): a zero-copy batch with the window pipeline runs the block steps of a burst in which every stream is
                                             FINE (MP1 routing, no acquisition kernels needed) as ONE launch whose workgroups -- pairs of symbol transforms and per-stream block
                                             steps -- hand over to each other, for stream sets of at least this many streams; 0 = never (two launches per step) */
    , NRSC5HIP_TUNE_LOOP_EXACT             /* FM Costas loops / CFO search (sync.c:90-136, 292-337) by the reference's own operations -- glibc's sincosf and atan2f restated
                                             bit for bit (fastmath.h), its float complex products, adjust_ref / reset_ref in place -- instead of the fast forms (v_sin / v_cos,
                                             a 4-term arc tangent, ~5e-7): 0 = never, 1 (default) = in every block that starts un-synchronised (the tracking pass over garbage and the
                                             CFO search, where a last-bit difference can be amplified into a different loop state), 2 = in every block */
    , NRSC5HIP_TUNE_HOST_CAPTURE           /* fast streaming seam, FM cu8 (round 6): 1 (default) = the pushes of a session stay, as they arrive, in a pinned device-mapped capture that
                                             the stream reads in place across PCIe (the zero-copy batch's kernels: half-band fused into the symbol transform) -- a push is one host
                                             memcpy, no decimator launch; 0 = pinned staging + decimator kernel into the device FIFO (rounds 3 - 5).  Identical records either way.
                                             >= 512: on, with that many KiB of capture buffer instead of 16 MiB (the live tail moves to the front when it is full).  One stream per
                                             engine reads such a capture (the first to push cu8 after its reset); cs16 / AM input and the batch entry points use the FIFO */
    , NRSC5HIP_TUNE_FOLD_REPORT            /* fast streaming seam: 1 (default) = a block step with nothing to launch behind the sync kernel (no P1 frame to decode, no extended sidebands: 15 of 16
                                             MP1 blocks) has the sync kernel post the step's report into pinned host memory itself; 0 = the report kernel as a launch of its own.  Identical records */
};
/* process-wide wall-clock totals of the streaming seam with p1_async = 0 (what the drop-in uses): [0] s copying pushes into pinned
 * staging, [1] s enqueueing H2D + decimator, [2] s enqueueing block steps, [3] s waiting for the device (one sync per block),
 * [4] pushes, [5] submissions, [6] block steps, [7] s fetching P1 frames */
void nrsc5hip_debug_seam_totals(double out[8], int reset);   /* totals of the CALLING THREAD's sessions */
/* ... [0] block steps left in flight (deferred wait), [1] read positions the host predicted wrongly (expected: 0), [2] steps submitted
 * without the P1 decode launches (no frame could complete), [3] P1 decodes launched after the fact (expected: 0) */
void nrsc5hip_debug_seam_counts(double out[6], int reset);   /* ... [4] block steps submitted ahead of the previous block's delivery, [5] pushes copied into a host-resident capture (NRSC5HIP_TUNE_HOST_CAPTURE) */
/* test / bench hygiene: overwrite every result buffer a pass writes (frame rings on the device and their pinned host mirror, record
 * rings) with a pattern no decode produces -- a check after the next pass can then only pass on bits written by that pass */
int nrsc5hip_debug_poison_results(nrsc5hip_engine *e);
/* segmented forward pass: segment boundaries checked / segments that had to be re-run since the engine was created */
int nrsc5hip_debug_fwd_stats(nrsc5hip_engine *e, int stats[2]);
/* dataflow bursts (NRSC5HIP_TUNE_FLOW_MIN): [0] bursts, [1] block steps issued as k_flow launches since the engine was created */
int nrsc5hip_debug_flow_stats(nrsc5hip_engine *e, long long stats[2]);
/* host-resident capture of the fast seam (NRSC5HIP_TUNE_HOST_CAPTURE): [0] sessions that bound the pinned capture, [1] captures turned back into the FIFO (cs16 push,
 * batch entry point, debug fetch), [2] times the live tail moved to the front of a full buffer, [3] the stream bound now (-1: none); and of NRSC5HIP_TUNE_FOLD_REPORT:
 * [4] block steps whose report the sync kernel posted itself */
int nrsc5hip_debug_host_capture_stats(nrsc5hip_engine *e, long long stats[5]);
/* K=9 decode in segment waves: [0] forward boundaries checked, [1] segments re-run, [2] traceback boundaries checked, [3] segments re-walked */
/* single-path traceback: [0] chunk boundaries checked, [1] chunks re-walked since the engine was created */
int nrsc5hip_debug_tb_stats(nrsc5hip_engine *e, int stats[2]);
int nrsc5hip_debug_k9_stats(nrsc5hip_engine *e, int stats[4]);
int nrsc5hip_debug_tune(nrsc5hip_engine *e, int knob, int value);
/* accumulated shader cycles per phase of the sync kernel for stream 0 (after nrsc5hip_debug_tune(e, NRSC5HIP_TUNE_SYNC_PHASES, 1)) in [0..7];
 * [8..15]: phases of the symbol kernel, filled only by a diagnostic build of the library (-DNRSC5HIP_MIXFFT_PHASES), else zero */
int nrsc5hip_debug_sync_phases(nrsc5hip_engine *e, long long *cycles16);
/* debugging aid: soft-bit matrix (16 x 23040 int8) and live FFT bins of a stream's latest block */
int nrsc5hip_debug_fetch(nrsc5hip_engine *e, int stream, int8_t *pm /* [368640] or NULL */, float *bins /* [32][534][2] or NULL */);

/* debugging aid: Costas loop state (sync_t.costas_freq / costas_phase) of the 534 live bins (2 x 267: lower sideband bins 478..744,
 * upper 1304..1570) of a stream */
int nrsc5hip_debug_fetch_costas(nrsc5hip_engine *e, int stream, float *freq /* [534] */, float *phase /* [534] */);

/* debugging aid: PX1 / PX2 soft bits of the stream's current block pair, [2 channels][2 blocks][4608] int8 */
int nrsc5hip_debug_fetch_px(nrsc5hip_engine *e, int stream, int8_t *pair /* [18432] */);

/* debugging aid: an AM stream's hard-symbol matrices (pl, pu, s, t: 4 x 6400 bytes; block bc of the L1 frame being received at bc * 800) */
int nrsc5hip_debug_fetch_am_sym(nrsc5hip_engine *e, int stream, uint8_t *sym /* [4][6400] */);

/* fresh-session state for every stream (input_reset on all of them) */
int nrsc5hip_reset_all(nrsc5hip_engine *e);

/* Per-kernel-class device timing, measured with HIP events recorded on the stream each kernel is
 * launched on.  enable: 1 start (and zero the accumulators), 0x100 | class start but time that class only (the events around
 * every launch of the block-step chain cost ~9 % of a batch pass), 0 stop (and zero), -1 just read.
 * total_ms / launches: arrays of NRSC5HIP_PROF_CLASSES entries (may be NULL). */
enum {
    NRSC5HIP_PROF_DECIMATE = 0, NRSC5HIP_PROF_ACQUIRE, NRSC5HIP_PROF_PREPARE, NRSC5HIP_PROF_MIXFFT,
    NRSC5HIP_PROF_SYNC, NRSC5HIP_PROF_P1_DEINT, NRSC5HIP_PROF_P1_VITERBI, NRSC5HIP_PROF_PIDS, NRSC5HIP_PROF_AM /* block steps */, NRSC5HIP_PROF_AM_DECODE /* window pipeline: the deferred decodes */,
    NRSC5HIP_PROF_P1_TRACEBACK /* P1_DEINT / P1_VITERBI (the forward trellis pass) / P1_TRACEBACK: the three stages of a P1 decode */,
    NRSC5HIP_PROF_FLOW /* dataflow bursts: up to 16 block steps of a stream set (symbol transforms + block steps) as one launch of k_flow */,
    NRSC5HIP_PROF_CLASSES
};
int nrsc5hip_profile(nrsc5hip_engine *e, int enable, double *total_ms, long long *launches);

/* test helpers: first n samples of a stream's Q15 FIFO slab; raw device allocation for batch tests */
int nrsc5hip_debug_fetch_q15(nrsc5hip_engine *e, int stream, long long n, int16_t *out /* [n][2] */);
void *nrsc5hip_debug_alloc_copy(const void *host, size_t nbytes);
void nrsc5hip_debug_free(void *dev);

/* ---- wideband channelizer (ABI 8): one SDR capture at any rate -> one reference-format cs16 stream per station -------------
 * Input: complex samples x[n] (n counted from the last create / reset) at Fs_in = rate_num / rate_den S/s, 744 187.5 <= Fs_in
 * <= 64e6, as cu8 (scaled (b - 127) * 64, U8_Q15 of defines.h:93), cs16 (as is) or cf32 (v * 32768).  Per channel k (1 <= K <= 512):
 *   mixer      x[n] * exp(-j 2 pi theta_k[n] / 2^32), theta_k[n] = n * s_k mod 2^32, s_k = round(f_k / Fs_in * 2^32): integer phase,
 *              no drift however long the session; the realised offset s_k * Fs_in / 2^32 is reported by nrsc5hip_chan_info
 *   resampler  output m at input time t_m = m * P / Q (P / Q = Fs_in / 744 187.5, reduced), floor(t_m) and (m P mod Q) / Q in 64-bit
 *              integers; y_k[m] = g_k * sum_n mixed[n] * h(t_m - n), h a Kaiser lowpass of support T input samples (passband
 *              +-0.1 dB to 198.5 kHz, >= 70 dB from 545.8 kHz), stored as a float32 table of L phases x T taps (nearest phase;
 *              nrsc5hip_chan_taps reads it back); samples before n = 0 are zero
 *   output     round to nearest, clamp to int16 (clamped samples counted per channel), interleaved cs16 at 744 187.5 S/s: the
 *              stream a tuner centred at f_k hands to nrsc5_pipe_samples_cs16 (a station at +f_k comes out at 0 Hz, unconjugated)
 * Output m exists once input floor(t_m) + T/2 has arrived: the output count depends on the total input only, and every output's
 * arithmetic on absolute indices only, so any chunking of the input (down to 1 sample) gives identical bytes.
 * The object runs on its own HIP stream on cfg.device (switched to and restored by every entry point, as for an engine); it is not
 * re-entrant.  nrsc5hip_chan_create rejects (NRSC5HIP_EINVAL) a rate out of range, a rate whose reduced ratio P / Q has a term of 2^31
 * or more (rate_den above ~1442 with terms prime to 1488375 * 2), |f_k| > Fs_in / 2 - 198.5 kHz, nchan outside 1..512 and an unknown
 * format. */
enum { NRSC5HIP_IQ_CU8 = 0, NRSC5HIP_IQ_CS16 = 1, NRSC5HIP_IQ_CF32 = 2 };
typedef struct nrsc5hip_chan_config {
    int device, format, nchan;
    long long rate_num, rate_den;        /* Fs_in = rate_num / rate_den S/s */
    const double *offset_hz;             /* [nchan] centre of each channel relative to the capture centre */
    const float *gain;                   /* [nchan] or NULL (1) */
} nrsc5hip_chan_config;
typedef struct nrsc5hip_chan nrsc5hip_chan;
int  nrsc5hip_chan_create(const nrsc5hip_chan_config *cfg, nrsc5hip_chan **out);
void nrsc5hip_chan_destroy(nrsc5hip_chan *c);
int  nrsc5hip_chan_reset(nrsc5hip_chan *c);                                    /* == a freshly created object */
/* realised_offset_hz[nchan] (may be NULL), taps = T, phases = L */
int  nrsc5hip_chan_info(nrsc5hip_chan *c, double *realised_offset_hz, int *taps, int *phases);
int  nrsc5hip_chan_taps(nrsc5hip_chan *c, float *table /* [phases][taps] */);
/* outputs per channel the next push of n_in samples yields (negative: error) */
long long nrsc5hip_chan_outputs_for(nrsc5hip_chan *c, long long n_in);
/* dev_in: device buffer of n_in complex samples of cfg.format; channel k's new outputs go to dev_out + k * out_stride_elems (int16
 * elements, >= 2 * out_capacity when nchan > 1).  NRSC5HIP_EOVERFLOW when they exceed out_capacity (samples per channel): the object is
 * then untouched.  Returns when the outputs are complete and dev_in is no longer read (a wait on the channelizer's own stream). */
int  nrsc5hip_chan_process(nrsc5hip_chan *c, const void *dev_in, long long n_in, int16_t *dev_out, long long out_stride_elems,
                           long long out_capacity, long long *n_out);
int  nrsc5hip_chan_clip_counts(nrsc5hip_chan *c, long long *counts /* [nchan], since create / reset */);
/* channelize and append channel k's new outputs to stream stream_ids[k] of an engine on the same device -- what
 * nrsc5hip_batch_append_cs16 of those outputs does; follow with nrsc5hip_batch_process.  The engine's stream waits for the channelizer
 * through an event (no device-wide sync), and the channelizer's next write to its staging buffer waits for the engine's append. When the
 * engine refuses the append (a stream id, q15_capacity: its error code is returned) the channelizer is left as before the call. */
int  nrsc5hip_chan_feed(nrsc5hip_chan *c, nrsc5hip_engine *e, const int *stream_ids, const void *dev_in, long long n_in);

/* ---- band scan (ABI 9): where are the HD stations of a wideband capture? -----------------------------------------------------
 * Input as for the channelizer: complex samples x[n] (n counted from the last create / reset) at Fs = rate_num / rate_den S/s,
 * 744 187.5 <= Fs <= 64e6, as cu8 ((b - 127) * 64), cs16 (as is) or cf32 (v * 32768).
 *   transform  nfft a power of two in 512..8192; cfg.nfft = 0 picks the smallest one >= Fs / 2000 Hz within that range
 *   segments   segment s covers samples [s H, s H + nfft), H = nfft / 2 (Welch, 50 % overlap), window periodic Hann
 *              w[j] = 0.5 - 0.5 cos(2 pi j / nfft); X_s[k] = sum_j w[j] x[s H + j] exp(-2 pi i j k / nfft)
 *   result     PSD[i] = sum_s |X_s[k]|^2 / (S * sum_j w[j]^2), i = (k + nfft/2) mod nfft: bin i lies at (i - nfft/2) * Fs / nfft, S is
 *              the number of complete segments since create / reset; white noise of variance v per sample gives PSD ~ v in every bin
 * Pushes may have any length (nfft - 1 samples of history are carried).  The same sequence of pushes gives the same bytes on every run;
 * another chunking of the same input computes the same segments and may add them in another order (all sums are double, as is the
 * transform).  The object runs on its own HIP stream on cfg.device (switched to and restored by every entry point); it is not
 * re-entrant.  nrsc5hip_scan_create rejects (NRSC5HIP_EINVAL) a rate that is not positive or out of range, an unknown format and an
 * nfft that is neither 0 nor a power of two in 512..8192.
 * Detector (host, double, deterministic; nrsc5hip_scan_detect_psd needs no device and no scan object):
 *   floor      the 20th percentile of the PSD: element (int)(0.2 * (nfft - 1)) of the sorted bins
 *   score(c)   for every bin centre c with |c| <= Fs/2 - 198.5 kHz: each sideband [c - 198 402, c - 129 361] and [c + 129 361,
 *              c + 198 402] Hz (carriers 356 and 546 of the 363.373 Hz grid) is split into four equal parts; the mean linear power of a
 *              part is the integral of the PSD, taken as constant across each bin, over the part's width; score = 10 log10(the least of
 *              the eight means / floor)
 *   picks      highest score first (ties: lower bin), none below threshold_db, none within +-min_separation_hz of an earlier pick
 * It is liberal on purpose (no edge or flatness test): two analog-only FM stations 400 kHz apart fill both windows of the slot between
 * them; nrsc5_amd/wideband.py: scan() confirms a nomination by decoding it. */
typedef struct nrsc5hip_scan_config {
    int device, format;
    long long rate_num, rate_den;        /* Fs = rate_num / rate_den S/s */
    int nfft;                            /* 0: the default for the rate */
} nrsc5hip_scan_config;
typedef struct nrsc5hip_scan_params {
    double threshold_db;                 /* 6 */
    double min_separation_hz;            /* 100e3 */
} nrsc5hip_scan_params;
typedef struct nrsc5hip_scan_station {
    double offset_hz;                    /* the bin centre picked, relative to the capture centre */
    float score_db, lower_db, upper_db;  /* lower / upper: mean power of the whole sideband over the floor */
    float floor_db;                      /* 10 log10 of the floor, in the PSD's units */
} nrsc5hip_scan_station;
typedef struct nrsc5hip_scan nrsc5hip_scan;
int  nrsc5hip_scan_create(const nrsc5hip_scan_config *cfg, nrsc5hip_scan **out);
void nrsc5hip_scan_destroy(nrsc5hip_scan *s);
int  nrsc5hip_scan_reset(nrsc5hip_scan *s);                                    /* == a freshly created object */
/* dev_in: device buffer of n_in complex samples of cfg.format; returns when it is no longer read */
int  nrsc5hip_scan_push(nrsc5hip_scan *s, const void *dev_in, long long n_in);
int  nrsc5hip_scan_info(nrsc5hip_scan *s, int *nfft, long long *segments, double *bin_hz);      /* any pointer may be NULL */
/* NRSC5HIP_EINVAL while no segment is complete */
int  nrsc5hip_scan_spectrum(nrsc5hip_scan *s, double *psd /* [nfft] */);
/* params NULL: the defaults.  Writes the first `max` picks (max >= 0) and sets *n to the number of picks found. */
int  nrsc5hip_scan_detect_psd(const double *psd, int nfft /* a power of two >= 16 */, double fs, const nrsc5hip_scan_params *params,
                              nrsc5hip_scan_station *stations_out, int max, int *n);
/* nrsc5hip_scan_spectrum followed by nrsc5hip_scan_detect_psd */
int  nrsc5hip_scan_detect(nrsc5hip_scan *s, const nrsc5hip_scan_params *params, nrsc5hip_scan_station *stations_out, int max, int *n);
/* Detector of analog FM carriers (ABI 21; host, double, deterministic, no device) on the same spectrum:
 *   floor      as above
 *   score(c)   for every bin centre c with |c| <= Fs/2 - 198.5 kHz (the channelizer can tune it): 10 log10(the mean power of
 *              [c - 50 kHz, c + 50 kHz], the PSD taken as constant across each bin, / floor)
 *   picks      highest score first (ties: lower bin), none below threshold_db, none within +-min_separation_hz of an earlier pick.  params
 *              NULL: 6 dB and 150 kHz, so that the shoulder of a strong carrier is not picked in front of a weak neighbour on the 200 kHz raster
 *   centre     offset_hz = the power centroid of max(PSD - floor, 0) over the bins whose centres lie in [c - 100 kHz, c + 100 kHz], added in bin
 *              order: sum f_i w_i / sum w_i (an FM signal's first spectral moment is its carrier); c itself when the weights sum to 0
 * Generous on purpose: the sidebands of a hybrid station are nominated too; the carrier measurement ("carrier quality" below; nrsc5_amd/
 * wideband.py: confirm_analog) removes them. */
typedef struct nrsc5hip_scan_fm_station {
    double offset_hz;                    /* the centroid, relative to the capture centre */
    double bin_hz;                       /* the bin centre picked */
    float score_db, floor_db;
} nrsc5hip_scan_fm_station;
int  nrsc5hip_scan_detect_fm_psd(const double *psd, int nfft /* a power of two >= 16 */, double fs, const nrsc5hip_scan_params *params,
                                 nrsc5hip_scan_fm_station *stations_out, int max, int *n);
/* nrsc5hip_scan_spectrum followed by nrsc5hip_scan_detect_fm_psd */
int  nrsc5hip_scan_detect_fm(nrsc5hip_scan *s, const nrsc5hip_scan_params *params, nrsc5hip_scan_fm_station *stations_out, int max, int *n);

/* ---- analog FM audio (ABI 16): the analog programme of every station's 744 187.5 S/s cs16 stream as 44.1 kS/s stereo PCM -----------
 * Input: per channel (1 <= nchan <= 512) the cs16 stream the channelizer makes, x[n] (n counted from the last create / reset, x[n] = 0 for
 * n < 0), Fs = 744 187.5 S/s.  Every quantity is a function of absolute sample indices; there is no recurrence and no loop filter, so any
 * chunking of a session (down to 1 sample) gives identical bytes.  Fs1 = Fs / 2 = 372 093.75 S/s; audio rate = Fs1 * 16 / 135 = 44 100 S/s.
 *   channel filter  z[m] = sum_i hA[i] x[2 m - i], i < 112: Kaiser lowpass (double on the host, stored float32, DC gain 1), +-0.1 dB to
 *                   95 kHz, >= 70 dB from 129 361 Hz (the first primary-main carrier).  In MP2 / MP3 / MP11 the extended carriers from
 *                   101.7 kHz lie inside the passband: inherent, the analog programme and they share those frequencies
 *   discriminator   d[m] = atan2(Im w, Re w) * Fs1 / (2 pi 75 000), w = z[m] conj z[m - 1]; d[0] = 0, and d[m] = 0 where w = 0 (silence in,
 *                   silence out); +-75 kHz -> +-1
 *   pilot           phi19(m) = 2 pi ((608 m) mod 11907) / 11907 (19 kHz exactly, 64-bit integers); block sums p[j] = sum over m in
 *                   [540 j, 540 j + 540) of d[m] exp(-j phi19(m)); smoothed p^[j] = sum over |w| <= 16 of win[w] p[j + w], win[w] =
 *                   0.5 (1 + cos(pi w / 17)), blocks in front of the stream zero; level a = 2 |p^| / 540 / sum(win); block j is stereo
 *                   when a >= pilot_min; subcarrier of block j: sub[m] = sin(2 phi19(m) + 2 theta_j), exp(j 2 theta_j) = -(p^ / |p^|)^2
 *   paths           sum S[m] = d[m]; difference D_j[m] = 2 (aq d[m - 1] + bq d[m] + aq d[m + 1]) sub[m] (0 in a mono block); (aq, bq, aq)
 *                   undoes the discriminator's droop sinc(f / Fs1) around the subcarrier: exact at 28 and 48 kHz
 *   resampler       audio output k of block j = k / 64 sits at t_k = 135 k / 16 Fs1 samples, i = floor(t_k), phase (135 k) mod 16 exactly:
 *                   y[k] = sum_j' tab[phase][j'] src[i - j'], j' < taps_audio, for src = S and src = D_j; the prototype (at 16 Fs1, DC gain
 *                   16) is a Kaiser lowpass (flat to 15 kHz, >= 60 dB from 19 kHz) convolved with the de-emphasis exp(-t / tau) sampled
 *                   at 16 Fs1 (its first sample halved) and cut below 2^-30; tau = 75 us, 50 us or 0 (none)
 *   output          L = S + D, R = S - D; int16 = round to nearest of (float32)(32767 gain) v, clamped (clamps counted per channel and
 *                   side), interleaved L, R
 * Audio block j (64 outputs) exists once input sample 1080 (j + 17) - 2 has arrived (nrsc5hip_fm_info: latency_in = 18 359 samples in front
 * of the first block): the smoothing window looks 16 blocks ahead.  There is no flush: the tail of a session stays undelivered.
 * The object runs on its own HIP stream on cfg.device; it is not re-entrant. */
typedef struct nrsc5hip_fm_config {
    int device, nchan;
    double deemphasis_us;                /* 75, 50 or 0 */
    double pilot_min;                    /* 0: the default, 0.03 (the nominal injection is 0.08 .. 0.10) */
    const float *gain;                   /* [nchan] or NULL (1) */
} nrsc5hip_fm_config;
typedef struct nrsc5hip_fm nrsc5hip_fm;
int  nrsc5hip_fm_create(const nrsc5hip_fm_config *cfg, nrsc5hip_fm **out);
void nrsc5hip_fm_destroy(nrsc5hip_fm *fm);
int  nrsc5hip_fm_reset(nrsc5hip_fm *fm);                                       /* == a freshly created object */
int  nrsc5hip_fm_info(nrsc5hip_fm *fm, int *taps_channel, int *taps_audio, int *phases, long long *latency_in);   /* any pointer may be NULL */
int  nrsc5hip_fm_taps(nrsc5hip_fm *fm, float *channel /* [taps_channel] or NULL */, float *audio /* [phases][taps_audio] or NULL */);
/* stereo frames per channel the next push of n_in samples yields (negative: error) */
long long nrsc5hip_fm_outputs_for(nrsc5hip_fm *fm, long long n_in);
/* channel k's n_in new cs16 samples at dev_in + k * in_stride_elems (device memory, 4-byte aligned, in_stride_elems even and >= 2 * n_in when
 * nchan > 1); its new frames (L, R) go to dev_out + k * out_stride_elems (>= 2 * out_capacity when nchan > 1).  NRSC5HIP_EOVERFLOW when
 * they exceed out_capacity (frames per channel): the object is then untouched.  Returns when the outputs are complete. */
int  nrsc5hip_fm_process(nrsc5hip_fm *fm, const int16_t *dev_in, long long in_stride_elems, long long n_in, int16_t *dev_out,
                         long long out_stride_elems, long long out_capacity, long long *n_out);
int  nrsc5hip_fm_clip_counts(nrsc5hip_fm *fm, long long *counts /* [nchan][2]: L, R, since create / reset */);
/* test hook (ABI 19): kernel launches the pushes have issued since create / reset -- per push the front end (when a d sample is new), the pilot
 * sums (a block complete), the audio (an audio block due) and the kept tails (always); with RDS also the matched filter (a grid point new) and,
 * when a window was decided, decisions, groups and the kept y; with the carrier measurement also, when a block completed, the block sums and the
 * report (which keeps the tails; the front end writes r in its one launch).  Reception steering adds no launch of its own: a steered object
 * issues what an object with the carrier measurement does, the block sums in front of the audio.  The stage hooks are not counted */
int  nrsc5hip_fm_debug_launches(nrsc5hip_fm *fm, long long *count);
/* level a and stereo flag of the last audio block delivered (0 before the first); either pointer may be NULL */
int  nrsc5hip_fm_pilot(nrsc5hip_fm *fm, float *level /* [nchan] */, int *stereo /* [nchan] */);
/* stage hook: d (host, [nchan][(n_in + 1) / 2]) and the block sums (host, [nchan][((n_in + 1) / 2) / 540][2], may be NULL) of n_in samples
 * taken as a whole session from n = 0; the object's own session is not touched */
int  nrsc5hip_stage_fm_mpx(nrsc5hip_fm *fm, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *d_out, float *psum_out);
/* nrsc5hip_chan_feed, and the demodulator over the same staged outputs before the staging buffer is written again: the channelized
 * samples never visit the host.  fm has the channelizer's nchan and device; channel k's new frames go to dev_audio + k * audio_stride_elems.
 * NRSC5HIP_EOVERFLOW (audio_capacity) and an append the engine refuses leave both objects as before the call. */
int  nrsc5hip_chan_feed_fm(nrsc5hip_chan *c, nrsc5hip_engine *e, const int *stream_ids, nrsc5hip_fm *fm, const void *dev_in, long long n_in,
                           int16_t *dev_audio, long long audio_stride_elems, long long audio_capacity, long long *n_audio);

/* ---- RDS / RBDS of the analog host (ABI 19): programme identification, station name, RadioText and clock from the 57 kHz subcarrier ----
 * Opt-in per analog FM object (nrsc5hip_fm_rds_enable); it then runs inside every nrsc5hip_fm_process / nrsc5hip_chan_feed_fm on the same
 * stream, from the discriminator output d[m] at Fs1 (the channel filter is flat to 95 kHz).  Every rate is exact on the Fs1 grid: 57 kHz is
 * 1824 / 11907 cycles per sample, a bit is 11907 / 38 samples, so bit timing is a function of absolute sample indices (64-bit integers): no
 * NCO, no loop filter, no recurrence in the signal path, and any chunking of a session gives identical bits, events and counters.
 *   baseband        v[m] = d[m] exp(-j 2 pi ((1824 m) mod 11907) / 11907).  The pilot is not used: detection is differential, the carrier's
 *                   phase drops out, and a station without a pilot decodes as well
 *   matched filter  on a grid of 8 points per bit: point r at t_r = 11907 r / 304 samples, i = floor(t_r), phase (11907 r) mod 304 exactly;
 *                   y[r] = sum_j tab[phase][j] v[i + j - 627], j < 1255 (every |m - t_r| <= 2 T, T the bit period; samples in front of the
 *                   stream zero); tab = g(tau + T / 4) w(tau) at tau = j - 627 - phase / 304: g(t) = h(t) - h(t - T / 2), h(t) =
 *                   sinc(4 t / T + 1/2) + sinc(4 t / T - 1/2) (the standard's cos(pi f T / 4) spectrum), w the Hann window over |tau| <= 2 T,
 *                   zero beyond; double on the host, stored float32
 *   timing          windows of 152 bits = 1216 grid points = 47 628 samples: E_w[s] = sum over the window's bits k of |y[8 k + s]|^2 (lane
 *                   8 g + s sums k = g, g + 8, .. in order, then a butterfly over g), s_w = argmax, ties to the lowest s; sampling points
 *                   8 k + s_w.  Seam to window w - 1: gap = 8 + s_w - s_{w-1}; gap < 4: the first point of w is dropped; gap > 12: one point
 *                   is inserted 8 grid steps behind the last point of w - 1
 *   decisions       data bit i = Re(y[r_i] conj y[r_{i-1}]) < 0 (differentially coherent detection of the differentially encoded stream);
 *                   the first point of a session gives no bit.  A window is decided once every y it reads exists: window w after
 *                   latency_in + 95 256 w input samples (nrsc5hip_fm_rds_info; latency_in = 96 431).  There is no flush
 *   blocks          (26, 16) code, generator x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1, offset words A 0x0FC, B 0x198, C 0x168, C' 0x350,
 *                   D 0x1B4: a word is valid with offset X when its remainder equals X.  Searching: every bit position is tested against
 *                   all five; sync when three valid words follow each other 26 bits apart in the cyclic order A, B, C or C', D (nothing is
 *                   corrected).  In sync: only the expected offset (C, then C' in the third place); a burst of at most correct_burst bits is
 *                   corrected by syndrome; sync is lost after 16 invalid blocks with no block valid as received between them (a corrected block
 *                   neither counts nor ends the run: behind a bit slip the shifted blocks have few syndromes, some of them correctable)
 *   groups          four blocks from an A on, all valid, else the group is dropped and counted; blocks between the sync and the first A
 *                   belong to no group
 *   content         PI (block A, and block C of version-B groups); PTY, TP (every group); TA, MS, DI and the name (0A / 0B: reported when all
 *                   four segments have arrived since the last reset or PI change and it differs from the last one reported); RadioText
 *                   (2A: 16 x 4 bytes, 2B: 16 x 2; a change of the A/B flag or of the version clears the buffer; reported when segments
 *                   0 .. L - 1 are present, L ending at the segment that holds 0x0D, else 16, and the text differs from the last one
 *                   reported); clock (4A: MJD, hour, minute, signed offset in half hours; once per distinct value); every other group is
 *                   counted by type and version.  A PI change forgets name and text.  Text is raw bytes. */
typedef struct nrsc5hip_rds_config {
    int raw_groups;                      /* also an NRSC5HIP_RDS_GROUP event per group */
    int correct_burst;                   /* 0 .. 2 bits corrected per block while in sync */
} nrsc5hip_rds_config;
enum { NRSC5HIP_RDS_PI = 1, NRSC5HIP_RDS_PS = 2, NRSC5HIP_RDS_RT = 3, NRSC5HIP_RDS_CLOCK = 4, NRSC5HIP_RDS_GROUP = 5 };
/* v: PI {pi}; PS {pi} + 8 bytes; RT {pi, A/B flag} + the text; CLOCK {mjd, hour, minute, offset}; GROUP {a, b, c, d}.  group: index of the
 * group since the last reset (dropped ones counted); bit: index of the bit that completed it */
typedef void (*nrsc5hip_rds_cb)(void *opaque, int channel, int kind, long long group, long long bit, const int32_t v[8], const uint8_t *data,
                                unsigned len);
typedef struct nrsc5hip_rds_info {
    int32_t pi;                          /* -1: none yet */
    int32_t pty, tp, ta, ms, di, synced;
    int32_t ps_len; uint8_t ps[8];       /* the last name reported; ps_len -1: none */
    int32_t rt_len, rt_ab; uint8_t rt[64];
    int32_t have_clock, mjd, hour, minute, offset_half_hours;
} nrsc5hip_rds_info;
/* bits, blocks valid / corrected / invalid, groups, groups dropped, syncs gained / lost, seam drops / inserts, groups by type and version
 * (0A, 0B, 1A, ..), events */
#define NRSC5HIP_RDS_NSTATS 43
/* cfg NULL: no raw groups, bursts of 2.  Only before the first nrsc5hip_fm_process / nrsc5hip_chan_feed_fm of the object; nrsc5hip_fm_reset
 * resets the RDS state as well */
int  nrsc5hip_fm_rds_enable(nrsc5hip_fm *fm, const nrsc5hip_rds_config *cfg);
/* the events appended since the last read, channel by channel, each channel's in order; -> events delivered, or < 0 */
int  nrsc5hip_fm_rds_read(nrsc5hip_fm *fm, nrsc5hip_rds_cb cb, void *opaque);
int  nrsc5hip_fm_rds_get(nrsc5hip_fm *fm, int channel, nrsc5hip_rds_info *out);
int  nrsc5hip_fm_rds_stats(nrsc5hip_fm *fm, int channel, long long stats[NRSC5HIP_RDS_NSTATS]);
int  nrsc5hip_fm_rds_info(nrsc5hip_fm *fm, int *taps, int *phases, int *points_per_bit, int *window_bits, long long *latency_in);   /* any pointer may be NULL */
int  nrsc5hip_fm_rds_taps(nrsc5hip_fm *fm, float *taps /* [phases][taps] */);
/* stage hook: n_in samples taken as a whole session from n = 0 -> on the host y [nchan][points][2], the window energies [nchan][windows][8],
 * s_w [nchan][windows], the decisions [nchan][windows][160] (one byte per bit) and their counts [nchan][windows], before any decoding; points =
 * ((304 (m - 628) + 303) / 11907) + 1 for m = (n_in + 1) / 2 >= 628, windows = points / 1216.  Any pointer may be NULL.  The object's own
 * session is not touched */
int  nrsc5hip_stage_rds_mf(nrsc5hip_fm *fm, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *y_out, float *energy_out,
                           int32_t *s_out, uint8_t *bits_out, int32_t *counts_out);
/* stage hook: bits (host, one byte each) fed straight to the group decoder of the listed channels (channels NULL: 0 .. n - 1); reset_at[i]
 * (or NULL): channel i's decoder is reset in front of that bit of the call (nbits[i]: behind the last; -1: never).  Events come with
 * nrsc5hip_fm_rds_read */
int  nrsc5hip_stage_rds_groups(nrsc5hip_fm *fm, int n, const int *channels, const uint8_t *const *bits, const int *nbits, const int *reset_at);

/* ---- carrier quality of the analog host (ABI 21): level, carrier-to-noise ratio and centre error of every channel's FM carrier ----------
 * Opt-in per analog FM object (nrsc5hip_fm_carrier_enable); it then runs inside every nrsc5hip_fm_process / nrsc5hip_chan_feed_fm on the same
 * stream.  Notation of "analog FM audio": z[m] the channel filter's output at Fs1, d[m] the discriminator, blocks of 540 Fs1 samples.  Every
 * quantity is a function of absolute sample indices, there is no recurrence, and every sum has a stated order: any chunking of a session gives
 * the same bits.  With the measurement disabled nothing changes: not a byte of d or of the audio, not the launch count.
 *   envelope        r[m] = |z[m]|^2 = fma(Re z, Re z, Im z Im z) in float32, from the z the discriminator uses
 *   block sums      for every complete block j, in double: s2[j] = sum r[m], s4[j] = sum r[m]^2 (the product is exact in double), s1[j] = sum d[m]
 *                   over m in [540 j, 540 j + 540); lane l of 64 takes m = 540 j + l + 64 i, i ascending, then an xor butterfly (32, 16, .. 1)
 *   windowed        of the last audio block delivered, ja: sum over |w| <= 16 of win[w] (s2, s4, s1)[ja + w], win the pilot's window as float32,
 *                   each product in double, blocks in front of the stream zero; lane w + 16 holds term w, then the butterfly.  count = the sum
 *                   of the 33 float32 window values in double (17 to rounding); it has the latency of the audio
 *   running         every complete block since create / reset, added one after the other in block order, in double; count = the blocks
 *   figures         on the host in double from a triple, the means per sample P = sum2 / (540 count), K = sum4 / (540 count):
 *                     S = sqrt(max(0, 2 P^2 - K))   carrier power: the second / fourth moment estimator, exact in expectation for a carrier of
 *                     N = P - S                     constant modulus in complex Gaussian noise (M2 = S + N, M4 = S^2 + 4 S N + 2 N^2)
 *                     level_db  = 10 log10(S / 32768^2)
 *                     cnr_db    = 10 log10(S / N), in the channel filter's noise bandwidth: white input noise of power v per sample leaves
 *                                 v sum hA[i]^2 in z (-5.34 dB for the 112 taps), so the figure is 5.34 dB above a CNR taken over the whole
 *                                 744 187.5 S/s
 *                     offset_hz = 75 000 sum1 / (540 count): the MPX has no DC, so the mean discriminator output is the centre error
 *                   S = 0 or P = 0: level_db = cnr_db = NRSC5HIP_FM_CARRIER_DB_MIN; N <= 0: cnr_db = NRSC5HIP_FM_CARRIER_DB_MAX; both figures
 *                   are clamped to that range: never NaN, never infinite.  count = 0 (no block yet): every field 0
 * Inherent: above about 40 dB the estimate saturates under modulation (its passage through the channel filter makes the envelope uneven; an
 * unmodulated carrier does not saturate), and a signal without a carrier -- noise, OFDM sidebands -- reads below 0 dB or at the lower clamp,
 * which is what makes the figure a detector of analog carriers. */
#define NRSC5HIP_FM_CARRIER_DB_MIN (-150.0)
#define NRSC5HIP_FM_CARRIER_DB_MAX 150.0
typedef struct nrsc5hip_fm_carrier_report {
    double sum2, sum4, sum1, count;      /* the triple and what it is divided by */
    double level_db, cnr_db, offset_hz;
} nrsc5hip_fm_carrier_report;
typedef struct nrsc5hip_fm_carrier_info {
    nrsc5hip_fm_carrier_report windowed, running;
    long long blocks, audio_blocks;      /* complete blocks and audio blocks delivered since create / reset */
} nrsc5hip_fm_carrier_info;
/* Only before the first nrsc5hip_fm_process / nrsc5hip_chan_feed_fm of the object; nrsc5hip_fm_reset keeps it enabled and zeroes the totals */
int  nrsc5hip_fm_carrier_enable(nrsc5hip_fm *fm);
/* NRSC5HIP_EINVAL on an object without the measurement.  Only the two triples per channel cross to the host */
int  nrsc5hip_fm_carrier(nrsc5hip_fm *fm, nrsc5hip_fm_carrier_info *out /* [nchan] */);
/* stage hook: r (host, [nchan][(n_in + 1) / 2]) and the block triples (host, [nchan][((n_in + 1) / 2) / 540][3]: s2, s4, s1; may be NULL) of
 * n_in samples taken as a whole session from n = 0; the object's own session is not touched, and the measurement need not be enabled */
int  nrsc5hip_stage_fm_carrier(nrsc5hip_fm *fm, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *r_out, double *sums_out);

/* ---- reception steering (ABI 22): stereo blend, high-cut and soft mute of the analog FM audio by the carrier quality of its own block ------
 * Opt-in per analog FM object (nrsc5hip_fm_steer_enable; it enables the carrier measurement when that is off).  Notation of "analog FM audio"
 * and "carrier quality": blocks of 540 Fs1 samples, audio block j = 64 outputs, win[w] the pilot's float32 window (|w| <= 16), (s2, s4, s1)[j]
 * the block triples.  Every quantity is a function of absolute block indices, there is no recurrence and no host round trip: any chunking of a
 * session gives identical bytes.  With steering off nothing changes: not a byte of the audio, not the order or the count of the launches.
 *   quality         of audio block j: W2_j = sum over |w| <= 16 of win[w] s2[j + w], W4_j likewise, in the arithmetic of the windowed report (each
 *                   product in double, blocks in front of the stream zero, lane w + 16 holds term w, the xor butterfly): for the last block of a
 *                   push they are the report's own bits.  c_j = the sum of (double)win[w] over the terms with j + w >= 0, same lanes, same
 *                   butterfly (not the constant 17: the first 16 blocks of a session would read as bad reception only because half their window
 *                   lies in front of the stream).  In double: kappa_j = W4_j (540 c_j) / (W2_j W2_j), q_j = min(1, max(0, 2 - kappa_j)) when
 *                   W2_j > 0, else 0.  This is (S / P)^2 of the second / fourth moment estimator; for a good carrier q ~ 1 - 2 N / S, so a ramp
 *                   linear in q is linear in the noise-to-carrier ratio, which the audio noise is proportional to
 *   ramps           a threshold of t dB CNR (in the channel filter's bandwidth, as cnr_db) is, on the host in double, rho = 10^(t / 10),
 *                   u = rho / (1 + rho), qt = u u; a ramp [lo_db, hi_db] is stored as float32 (q_lo, inv = 1 / (q_hi - q_lo)); on the device in
 *                   float32 f_j = min(1, max(0, ((float)q_j - q_lo) inv)).  blend b_j = f_j (weight of the difference path; 18 .. 30 dB);
 *                   high-cut h_j = f_j (weight of the wide table against the narrow one; 10 .. 20 dB); mute g_j = fma(f_j, 1 - floor, floor)
 *                   (2 .. 8 dB, floor = 10^(mute_floor_db / 20), -20 dB), which is exactly 1 at f_j = 1.  A control that is off has factor 1
 *   inside a block  the controls move linearly from block j - 1's value to block j's: for output i = k mod 64,
 *                   c(k) = fma(c_j - c_{j-1}, (float)(i + 1) / 64, c_{j-1}), c_{-1} = c_0.  Only blocks up to j + 16 are read: the audio's latency
 *   narrow table    a second prototype built like the first (same Kaiser attenuation and length, same de-emphasis convolution and cut, DC gain
 *                   16), pass edge 4 kHz, stop edge 8 kHz: the transition width and with it taps_audio and phases are unchanged
 *   output          Sw, Dw the two sums of "resampler", Sn, Dn the same sums on the narrow table; S' = fma(h, Sw, (1 - h) Sn), D' likewise;
 *                   L = (S' + b D') g, R = (S' - b D') g, then scale, round, clamp and clip count as before.  In a block whose two end values of
 *                   h are 1 the narrow sums are not formed (Sn = Dn = 0); in one whose two end values of b are 0 the difference path is not
 *                   formed (D = 0, L == R byte for byte); with b = h = g = 1 at both ends the block's bytes are the unsteered ones.  A mono block
 *                   (pilot below pilot_min) has D = 0 as before */
enum { NRSC5HIP_FM_STEER_BLEND = 1, NRSC5HIP_FM_STEER_HIGHCUT = 2, NRSC5HIP_FM_STEER_MUTE = 4, NRSC5HIP_FM_STEER_ALL = 7 };
typedef struct nrsc5hip_fm_steer_config {
    unsigned controls;                   /* NRSC5HIP_FM_STEER_* or'ed; a control that is off has factor 1 */
    double blend_db[2], highcut_db[2], mute_db[2];   /* [lo_db, hi_db], hi > lo, finite */
    double mute_floor_db;                /* <= 0 */
} nrsc5hip_fm_steer_config;
typedef struct nrsc5hip_fm_steer_info { float q, blend, highcut, mute; } nrsc5hip_fm_steer_info;
/* cfg NULL: every control, blend 18 .. 30 dB, high-cut 10 .. 20 dB, mute 2 .. 8 dB with a floor of -20 dB.  Only before the first
 * nrsc5hip_fm_process / nrsc5hip_chan_feed_fm of the object and only once; nrsc5hip_fm_reset keeps it enabled */
int  nrsc5hip_fm_steer_enable(nrsc5hip_fm *fm, const nrsc5hip_fm_steer_config *cfg);
/* q and the three factors at the end of the last audio block delivered (all 0 before the first).  NRSC5HIP_EINVAL on an unsteered object */
int  nrsc5hip_fm_steer(nrsc5hip_fm *fm, nrsc5hip_fm_steer_info *out /* [nchan] */);
/* the narrow table, laid out as nrsc5hip_fm_taps' audio table */
int  nrsc5hip_fm_steer_taps(nrsc5hip_fm *fm, float *audio_narrow /* [phases][taps_audio] */);
/* stage hook: (q, b, h, g) of every audio block of n_in samples taken as a whole session from n = 0 (host, [nchan][audio blocks][4], audio
 * blocks = max(0, ((n_in + 1) / 2) / 540 - 16)); the object's own session is not touched, and its launches are not counted */
int  nrsc5hip_stage_fm_steer(nrsc5hip_fm *fm, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *out);

/* ---- EAS alerts (SAME) of the analog host (ABI 23): the headers and end-of-message bursts of the Emergency Alert System in the programme audio ----
 * Opt-in per analog FM object (nrsc5hip_fm_same_enable); it then runs inside every nrsc5hip_fm_process / nrsc5hip_chan_feed_fm on the same
 * stream, from the discriminator output d[m] at Fs1 = 372 093.75 S/s (before de-emphasis).  SAME is AFSK at 3125 / 6 bit/s: mark (1) 6250 / 3 Hz,
 * four cycles per bit, space (0) 1562.5 Hz, three cycles per bit; bytes of 8 bits, the least significant first, no start or stop bits; a burst
 * is 16 bytes 0xAB and then ASCII: the header ZCZC-ORG-EEE-PSSCCC(-PSSCCC ..)+TTTT-JJJHHMM-LLLLLLLL- or the end of message NNNN, each sent three
 * times about 1 s apart.  On the Fs1 grid every rate is exact: a bit is 35721 / 50 samples, mark 200 / 35721 and space 150 / 35721 cycles per
 * sample, so timing is a function of absolute sample indices (64-bit integers): no NCO, no loop filter, no recurrence in the signal path, and
 * any chunking of a session gives identical bits, events and counters.  With SAME off nothing changes: no byte, no event, no launch count.
 *   tone sums       a grid of 8 points per bit: point r starts at g(r) = floor(35721 r / 400).  Segment sums, f = 1 (mark, k_1 = 200) and
 *                   f = 0 (space, k_0 = 150): c_f[r] = sum over m = g(r) .. g(r + 1) - 1 (89 or 90 samples) of
 *                   d[m] exp(-j 2 pi ((k_f m) mod 35721) / 35721), from one table of 35 721 (cos, sin) pairs computed in double and stored
 *                   float32; in float32, m ascending, Re += fma(d, cos, .), Im likewise with sin, negated at the end.  Bit sums
 *                   C_f[r] = c_f[r] + c_f[r + 1] + .. + c_f[r + 7], added in that order: exactly one bit length from g(r).  Decision value
 *                   q[r] = (Re C_1^2 + Im C_1^2) - (Re C_0^2 + Im C_0^2)
 *   timing          windows of 64 bits = 512 grid points: M_w[s] = sum over k < 64 of |q[512 w + 8 k + s]| (lane 8 g + s sums k = g, g + 8, ..
 *                   in order, then a butterfly over g), s_w = argmax, ties to the lowest s; sampling points 512 w + 8 k + s_w.  Seam to
 *                   window w - 1: gap = 8 + s_w - s_{w-1}; gap < 4: the first point of w is dropped; gap > 12: one point is inserted 8 grid
 *                   steps behind the last point of w - 1.  Every point yields a bit: the first window of a session has 64
 *   decisions       bit = 1 where q > 0.  A window is decided once every c it reads exists, c[512 w + 518] the last: window w after
 *                   2 floor(35721 (512 w + 519) / 400) - 1 input samples (latency_in of nrsc5hip_fm_same_info: window 0, 92 693).  No flush
 *   framing         per channel, in order over the bit stream; bit positions count from the last reset.  Search: a position matches when the
 *                   16 bits that end there are 0xAB 0xAB; a match while not in a message sets the byte boundary and enters preamble (and is
 *                   counted, and remembered as the burst's preamble match, when it comes from search).  Preamble: whole bytes; 0xAB stays, Z or
 *                   N opens a message, any other byte goes back to search.  Message: bytes accumulate; abort, counted, on a byte outside
 *                   0x20 .. 0x7E, when the first four bytes are neither ZCZC nor NNNN, and at 268 bytes; NNNN is complete at four bytes,
 *                   ZCZC.. at the third '-' behind the first '+'.  A complete burst is an NRSC5HIP_SAME_BURST event; the search resumes
 *   vote            a burst joins the current group when the group holds one or two bursts of its kind (header, end of message) and its
 *                   preamble match lies at most 2604 bits (5 s) behind the last bit of the group's newest burst; else it opens a new group.
 *                   One NRSC5HIP_SAME_MESSAGE event per group: the first time a burst equals an earlier one of the group byte for byte, or at
 *                   the third burst when all three have one length and every byte position a 2-of-3 majority (the text is the majority's).
 *                   A group that never agrees is counted when its third burst fails or when the next group opens
 * The fields of a header are not parsed on the device. */
#define NRSC5HIP_SAME_TEXT_MAX 268
typedef struct nrsc5hip_same_config {
    int burst_events;                    /* 1: also an NRSC5HIP_SAME_BURST event per burst; 0: messages only */
} nrsc5hip_same_config;
enum { NRSC5HIP_SAME_BURST = 1, NRSC5HIP_SAME_MESSAGE = 2 };
enum { NRSC5HIP_SAME_HEADER = 1, NRSC5HIP_SAME_EOM = 2 };
/* first, last: bit index of the first bit of the burst's text and of its last bit (MESSAGE: of the burst that decided it).  v: BURST {kind
 * (NRSC5HIP_SAME_HEADER / _EOM), place in its group 1 .. 3, bits from the preamble match to the first bit}; MESSAGE {kind, bursts of the group
 * so far}.  data: the text */
typedef void (*nrsc5hip_same_cb)(void *opaque, int channel, int kind, long long first_bit, long long last_bit, const int32_t v[8], const uint8_t *data,
                                 unsigned len);
typedef struct nrsc5hip_same_info {
    int32_t text_len;                    /* the last message; -1: none yet */
    int32_t kind;                        /* NRSC5HIP_SAME_HEADER / _EOM, 0: none */
    long long first_bit, last_bit;       /* of the burst that decided it; -1: none */
    int32_t group_bursts, group_kind;    /* the current group */
    int32_t in_message, pad;             /* the framer is inside a message */
    uint8_t text[272];
} nrsc5hip_same_info;
/* bits, preamble matches, bursts complete, bursts aborted, groups with a message, groups without, end-of-message messages, seam drops, seam
 * inserts, events */
#define NRSC5HIP_SAME_NSTATS 10
/* cfg NULL: burst events on.  Only before the first nrsc5hip_fm_process / nrsc5hip_chan_feed_fm of the object; nrsc5hip_fm_reset resets the
 * SAME state as well */
int  nrsc5hip_fm_same_enable(nrsc5hip_fm *fm, const nrsc5hip_same_config *cfg);
/* the events appended since the last read, channel by channel, each channel's in order; -> events delivered, or < 0 */
int  nrsc5hip_fm_same_read(nrsc5hip_fm *fm, nrsc5hip_same_cb cb, void *opaque);
int  nrsc5hip_fm_same_get(nrsc5hip_fm *fm, int channel, nrsc5hip_same_info *out);
int  nrsc5hip_fm_same_stats(nrsc5hip_fm *fm, int channel, long long stats[NRSC5HIP_SAME_NSTATS]);
int  nrsc5hip_fm_same_info(nrsc5hip_fm *fm, int *table, int *points_per_bit, int *window_bits, long long *latency_in);   /* any pointer may be NULL */
int  nrsc5hip_fm_same_table(nrsc5hip_fm *fm, float *cs /* [table][2]: cos, sin */);
/* stage hook: n_in samples taken as a whole session from n = 0 -> on the host c [nchan][segments][4] (Re c_1, Im c_1, Re c_0, Im c_0), q
 * [nchan][windows][512], the metrics [nchan][windows][8], s_w [nchan][windows], the decisions [nchan][windows][72] (one byte per bit) and
 * their counts [nchan][windows], before any framing; segments = (400 (m + 1) - 1) / 35721 for m = (n_in + 1) / 2, windows =
 * (segments - 7) / 512 (0 below 7).  Any pointer may be NULL.  The object's own session is not touched */
int  nrsc5hip_stage_same_tones(nrsc5hip_fm *fm, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *c_out, float *q_out,
                               float *metric_out, int32_t *s_out, uint8_t *bits_out, int32_t *counts_out);
/* stage hook: bits (host, one byte each) fed straight to the framer of the listed channels (channels NULL: 0 .. n - 1); reset_at[i] (or NULL):
 * channel i's framer and vote are reset in front of that bit of the call (nbits[i]: behind the last; -1: never).  Events come with
 * nrsc5hip_fm_same_read */
int  nrsc5hip_stage_same_frames(nrsc5hip_fm *fm, int n, const int *channels, const uint8_t *const *bits, const int *nbits, const int *reset_at);

/* ---- reception impairments of the analog host (ABI 24): multipath and adjacent-channel detectors of every channel's FM carrier --------------
 * Opt-in per analog FM object (nrsc5hip_fm_impair_enable; it enables the carrier measurement when that is off).  It then runs inside every
 * nrsc5hip_fm_process / nrsc5hip_chan_feed_fm on the same stream, two launches per push that completes a block.  Notation of "carrier quality":
 * blocks of 540 Fs1 samples, r[m] the envelope, d[m] the discriminator, win[w] the pilot's window as float32 (|w| <= 16).  Every quantity is a
 * function of absolute sample indices, there is no recurrence and every sum has a stated order: any chunking of a session gives the same bits.
 * With the measurement off nothing changes: not a byte of d, of the audio or of any report, not the launch count.
 *   amplitude       e[m] = sqrtf(r[m] * r[m - 1]) in float32 (the product rounded to float32, then the square root), e[0] = 0: the modulus of
 *                   z[m] conj z[m - 1], whose angle is d[m], so both signals sit at m - 1/2.  The square root is the correctly rounded one
 *                   (IEEE 754 sqrt: the device's sqrtf under hipcc's default of correctly rounded float32 division and square root; the tests
 *                   compare every e with the correctly rounded root of the library's own r, bit for bit)
 *   multipath sums  for every complete block j, in double, with x = d[m], y = e[m], over m in [540 j, 540 j + 540): the eight sums of
 *                   x, x2 = x x, x3 = x2 x, x4 = x2 x2, y, x y, x2 y, y y (x x, x y and y y are exact in double; the others round once per
 *                   product); lane l of 64 takes m = 540 j + l + 64 i, i ascending, then an xor butterfly (32, 16, .. 1): the carrier triples' order
 *   band-pass       hU: 63 taps, linear phase, hU[i] = (2 f2 sinc(2 f2 t) - 2 f1 sinc(2 f1 t)) kaiser(i; beta 8), t = i - 31, f1 = 100 kHz / Fs1,
 *                   f2 = 170 kHz / Fs1, designed in double, stored as float32 (nrsc5hip_fm_impair_taps).  eu[m] = sum_i hU[i] e[m - i],
 *                   du[m] = sum_i hU[i] d[m - i], each one float32 chain acc = fmaf(hU[i], e[m - i], acc) from acc = 0, i ascending; samples
 *                   in front of the stream are zero
 *   adjacent sums   per block, in double and in the order above: Cee = sum eu eu, Cdd = sum du du, Ced = sum eu du (every product exact)
 *   windowed        of the last audio block delivered, ja: sum over |w| <= 16 of win[w] v[ja + w] for each of the eleven sums v, each product
 *                   in double, blocks in front of the stream zero; lane w + 16 holds term w, then the butterfly.  count = the sum of the 33
 *                   float32 window values in double, as in the carrier report
 *   running         every complete block since create / reset, added one after the other in block order, in double; count = the blocks.  It
 *                   includes block 0, where the channel filter turns on (x[n] = 0 for n < 0): a step of e and a jump of d that weigh on the
 *                   running figures of a short session (an unmodulated carrier of 111 blocks reads a running explained of 0.56 at depth
 *                   0.016 and a windowed one of exactly 0).  Judge reception by the windowed report; the verdict thresholds are set for it
 *   figures         on the host, in double, from a set of sums and its count; every line is one statement, evaluated as written (no fused
 *                   multiply-add), so that an implementation in IEEE double agrees bit for bit but for log10:
 *                     n   = 540 count
 *                     mx  = sx / n, m2 = sxx / n, m3 = sxxx / n, m4 = sxxxx / n, my = sy / n, mxy = sxy / n, mxxy = sxxy / n, myy = syy / n
 *                     q   = mx mx
 *                     u2  = m2 - q                                              the centred moments of x
 *                     u3  = (m3 - (3 mx) m2) + (2 mx) q
 *                     u4  = ((m4 - (4 mx) m3) + (6 q) m2) - (3 q) q
 *                     cu  = mxy - mx my                                         cov(x - mx, y)
 *                     cv  = ((mxxy - (2 mx) mxy) + q my) - u2 my                cov((x - mx)^2, y)
 *                     k   = u4 - u2 u2
 *                     det = u2 k - u3 u3                                        of the normal equations of y - my ~ b1 (x - mx) + b2 ((x - mx)^2 - u2)
 *                     tot = myy - my my                                         total variance of y per sample
 *                     b1  = (cu k - cv u3) / det,  b2 = (cv u2 - cu u3) / det
 *                     res = tot - (b1 cu + b2 cv)                               residual variance per sample
 *                     explained = min(1, max(0, 1 - res / tot))
 *                     depth     = sqrt(max(0, tot - res)) / my                  rms of the fitted envelope variation over the mean envelope
 *                     c2 = b2,  c1 = b1 - (2 b2) mx,  c0 = (my - b1 mx) + b2 (q - u2)      y ~ c0 + c1 x + c2 x^2
 *                     slope     = c1 / c0  (per 75 kHz: x = 1 is 75 kHz),  curvature = c2 / c0;  both 0 unless c0 > 0
 *                   no fit -- explained = depth = slope = curvature = 0 -- unless my > 0, tot > 0, u2 >= NRSC5HIP_FM_IMPAIR_MOD_MIN (an rms
 *                   deviation of 75 Hz: an unmodulated carrier has no frequency to fit against) and det >= NRSC5HIP_FM_IMPAIR_MOD_MIN u2 u2 u2
 *                   (a near-singular system; a Gaussian x has det = 2 u2^3, one tone 0.5 u2^3), and every intermediate is finite
 *                     usn_db    = 10 log10(cdd / n)                             power of d in 100 .. 170 kHz ("ultrasonic noise"), 0 dB = 75 kHz rms
 *                     ripple_db = 10 log10((cee / n) / (my my))                 power of e in that band over the squared mean amplitude
 *                     rho       = ced / sqrt(cee cdd), clamped to [-1, 1]; 0 when cee or cdd is 0
 *                   the dB figures are NRSC5HIP_FM_CARRIER_DB_MIN when their argument is not positive and are clamped to _MIN .. _MAX: never
 *                   NaN, never infinite.  count = 0 (no block yet): every field 0
 *   verdict         NRSC5HIP_FM_IMPAIR_MULTIPATH when explained >= explained_min and depth >= depth_min; NRSC5HIP_FM_IMPAIR_ADJACENT when
 *                   |rho| >= rho_min, then side = +1 (rho > 0: the neighbour is above) or -1 (below), else side = 0.  Both can hold at once
 * Why: multipath is frequency-selective fading, so the amplitude becomes a function of the instantaneous frequency; a neighbour on one side adds
 * a beat that shows in the amplitude and in the frequency in phase (above) or in antiphase (below); white noise does neither.
 * Limit: a neighbour's carrier, 200 kHz away, lies in the channel filter's stop band; what the detector sees is the part of the neighbour's spectrum
 * that its own modulation swings below 129 kHz.  rho therefore grows with the neighbour's deviation as well as with its level: on the float64 model
 * a neighbour 10 dB below the carrier reads |rho| 0.80 when modulated close to full deviation, 0.43 .. 0.50 -- under the default rho_min -- when
 * modulated at about half of it, and 0.00 when silent, at any level.  A quiet or weak neighbour is missed; lower rho_min to trade this against
 * false alarms (noise alone: |rho| <= 0.03 in the window of 33 blocks) */
enum { NRSC5HIP_FM_IMPAIR_MULTIPATH = 1, NRSC5HIP_FM_IMPAIR_ADJACENT = 2 };
#define NRSC5HIP_FM_IMPAIR_TAPS 63
#define NRSC5HIP_FM_IMPAIR_NSUMS 11
#define NRSC5HIP_FM_IMPAIR_MOD_MIN 1e-6
typedef struct nrsc5hip_fm_impair_config {
    double explained_min;                /* 0 .. 1; default 0.5 */
    double depth_min;                    /* >= 0, finite; default 0.05 */
    double rho_min;                      /* 0 .. 1; default 0.5 */
} nrsc5hip_fm_impair_config;
typedef struct nrsc5hip_fm_impair_report {
    double sx, sxx, sxxx, sxxxx, sy, sxy, sxxy, syy, cee, cdd, ced, count;      /* the eleven sums and what they are divided by (in blocks) */
    double explained, depth, slope, curvature, usn_db, ripple_db, rho;
    int32_t verdict, side;               /* NRSC5HIP_FM_IMPAIR_* or'ed; +1, -1 or 0 */
} nrsc5hip_fm_impair_report;
typedef struct nrsc5hip_fm_impair_info {
    nrsc5hip_fm_impair_report windowed, running;
    long long blocks, audio_blocks;      /* complete blocks and audio blocks delivered since create / reset */
} nrsc5hip_fm_impair_info;
/* cfg NULL: the defaults.  Only before the first nrsc5hip_fm_process / nrsc5hip_chan_feed_fm of the object and only once; thresholds that are
 * not finite or out of range are refused; nrsc5hip_fm_reset keeps it enabled and zeroes the totals */
int  nrsc5hip_fm_impair_enable(nrsc5hip_fm *fm, const nrsc5hip_fm_impair_config *cfg);
/* NRSC5HIP_EINVAL on an object without the measurement.  Only the two sets of sums per channel cross to the host */
int  nrsc5hip_fm_impair(nrsc5hip_fm *fm, nrsc5hip_fm_impair_info *out /* [nchan] */);
/* hU as stored; the measurement need not be enabled */
int  nrsc5hip_fm_impair_taps(nrsc5hip_fm *fm, float *hu /* [NRSC5HIP_FM_IMPAIR_TAPS] */);
/* stage hook: e, eu, du (host, each [nchan][540 blocks], blocks = ((n_in + 1) / 2) / 540: the samples of the complete blocks; any may be NULL)
 * and the block sums (host, [nchan][blocks][11] in the order of nrsc5hip_fm_impair_report; may be NULL) of n_in samples taken as a whole session
 * from n = 0; the object's own session is not touched, the measurement need not be enabled, and the launches are not counted */
int  nrsc5hip_stage_fm_impair(nrsc5hip_fm *fm, const int16_t *dev_in, long long in_stride_elems, long long n_in, float *e_out, float *eu_out,
                              float *du_out, double *sums_out);

#ifdef __cplusplus
}
#endif
#endif /* NRSC5HIP_H_ */
