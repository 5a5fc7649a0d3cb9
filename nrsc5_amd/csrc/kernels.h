// Host-callable launchers for the gfx950 kernels (one .hip file per pipeline stage).
#pragma once
#include "nrsc5hip.h"
#include "nrsc5_dev.h"

namespace nrsc5 {

// Read-only device tables built once per engine (engine.hip: build_tables()).
struct DevTables {
    const uint16_t *deint_lut;       // [384] byte q of a 384-byte depunctured run -> block*720 + part*36, 0xffff = erasure
    const uint16_t *pids_gather;     // [16][PIDS_CODED] index inside block bc (decode.c:324-342)
    const uint32_t *eq_cell;         // [11520] MP1 data cell c = ((side * 10 + part) * 32 + n) * 18 + k - 1, packed: live bin | n << 10 | low ref << 15 |
                                     //         high ref << 20 | k << 25 | side << 30 (adjust_data's operands, sync.c:263-282)
    const uint16_t *eq_out;          // [11520] where the cell's soft-bit pair goes inside the block's interleaver rows (sync.c:514-536)
    const uint32_t *scr_p1;          // [P1_WORDS] packed scrambler stream (decode.c:279-294)
    const uint32_t *scr_pids;        // [3]
    const float2 *twiddle;           // [2048] e^{-2 pi i k / 2048}
    const float2 *twiddle_a;         // [7][256] the same values in the order the FFT's first exchange reads them: [k1 - 1][r] = twiddle[(k1 r) & 2047]
    const float *shape;              // [2160] pulse shape (acquire.c:322-331)
    const int16_t *hb_q15;           // [4]  half-band taps, window order
    const int16_t *acq_q15;          // [17] acquisition FIR taps, [1..16] used
    const uint32_t *px_delay_wide;   // [9216] interleaver IV write-to-read delay per position of a block pair, MP3 / MP11
    const uint32_t *px_delay_narrow; // [4608] same for MP2
    const uint32_t *am_deint_p1;        // [90000] source of every P1 trellis input (interleaver_ma1 folded into a table, see build_tables)
    const uint32_t *am_deint_p3_ma3;    // [90000] same for the MA3 P3 code word
    const uint32_t *am_deint_p3_ma1;    // [72000] same for the MA1 P3 code word
    const int16_t *am_acq_q15;       // [17] AM acquisition FIR taps (acquire.c:63-96)
    const float *am_shape;           // [270] AM pulse shape (acquire.c:333-342)
    const float2 *am_twiddle;        // [256] e^{-2 pi i k / 256}
};

// Engine-wide device buffers (slabs indexed by stream).
struct DevBuffers {
    StreamState *state;              // [S]
    StreamState *ckpt;               // [S][NWIN] replay: the stream's state right after the block that completed the P1 frame of decode
                                     // window w (slot w % NWIN), before the next block's bookkeeping; null unless p1_async && l2_feedback
    c16 *q15;                        // [S][q15_cap]
    long long q15_cap;
    c16 *acq_win;                    // [S][WIN_N]   zero-copy batch only: decimated acquisition window of streams that are not FINE
    c16 *acq_filt;                   // [S][WIN_N]   acquisition FIR output
    int *acq_list;                   // [S + 1]      streams that need the acquisition kernels this step (k_acq_list); [S] = how many
    float2 *acq_sums;                // [S][SYM_N]
    float2 *bins;                    // [S][NSYM][LIVE_N]
    float2 *cfo_snap;                // [S][LIVE_N][11]  the CFO search's loop-state snapshots (k_sync: one per visit of a live bin)
    float *cfo_phase;                // [S][NSYM][LIVE_N]  exact CFO search (loop_exact): phases[][] of the visit in progress, one column per live bin
    int loop_exact;                  // 0: fast loop arithmetic, 1: the reference's own operations in blocks that start un-synchronised, 2: in every block (sync_body.h)
    float2 *nco_tab;                 // [S][NSYM][SYM_N]  the reference's oscillator sample by sample for a block that runs in exact mode (k_nco_exact -> k_mixfft); null: closed form only
    int nco_policy;                  // NCO_*: which blocks of a freshly reset stream advance the oscillator by the reference's float recurrence
    int8_t *pm;                      // [S][NPM][PM_FRAME]  soft-bit interleaver matrices (one per frame in flight)
    int8_t *pids_stage;              // [S][NWIN][16][240]  depunctured PIDS soft bits awaiting k_pids_decode
    int *pids_rec;                   // [S][NWIN][16]     record index of each staged PIDS frame, -1 = empty
    int *coded;                      // [NAUX][S][P1_LEN]  depunctured P1 trellis input, one dword per step (s0 | s1 << 8 | s2 << 16), one per decode lane
    uint32_t *dec;                   // [NAUX][S][2 * (P1_LEN + 64)]  survivor decisions: per 32 steps one history word per lane (viterbi_v3.h)
    int nstreams_alloc;              // S
    uint8_t *tbmap;                  // [NAUX][S][2285 * 64]  traceback chunk maps (start lane per end lane)
    int *fwd_meta;                   // [NAUX][S][VIT3_GMAX][512]  segmented forward pass: per segment the metric snapshot [64], end metrics [64] and the
                                     //                     history scratch of its speculative warm-up [384] (viterbi_v3.h)
    int *fwd_stats;                  // [2] segment boundaries checked / segments repaired since the engine was created
    int *tb_stats;                   // [2] single-path traceback: chunk boundaries checked / chunks re-walked since the engine was created
    uint32_t *p1_ring;               // [S][p1_slots][P1_WORDS]
    uint32_t *p1_mirror;             // same layout in pinned host memory (device-visible), written beside p1_ring by the FM traceback once
                                     // nrsc5hip_batch_fetch_view has set it up; null before
    int p1_slots;
    BlockRecord *records;            // [S][rec_cap]
    int rec_cap;
    int *counters;                   // per burst: [0] blocks prepared, [1] not-FINE streams seen (host: keep launching the acquisition kernels),
                                     // [2] streams that need the PX kernels, [3] streams rewound by k_rollback
    long long *sync_phase_cycles;    // [16] optional: accumulated shader cycles per k_sync phase (stream 0 only) in [0..7]; [8..15]: k_mixfft's phases in the diagnostic build; or null
    // extended sidebands
    int8_t *px_mem;                  // [S][2][PX_MEM]           interleaver IV memories of PX1, PX2
    int8_t *px_pair;                 // [S][2][2 * PX_MAX]       soft bits of the current block pair
    int8_t *px_stage;                // [S][NWIN][8][2][PX_DEPUNCT]  depunctured trellis inputs awaiting k_px_decode
    PxJob *px_job;                   // [S][NWIN][8][2]
    unsigned long long *px_dec;      // [NAUX][S][16][PX_MAX + 64] survivor decisions
    uint32_t *px_ring;               // [S][px_slots][2][PX_WORDS]
    int px_slots;
    // AM (null unless the engine was created with am_enable)
    AmStream *am;                    // [S]
    uint8_t *am_sym;                 // [S][4][AM_SYMS]   hard symbols of the current L1 frame: pl, pu, s, t
    uint8_t *am_q;                   // [S][3][2][AM_VIT]  3-frame diversity delay of the ml / mu (/ eml / emu) bits: one cell per trellis input of the P1 / P3 code word, keyed by the input's index (coalesced; the reference's line / position numbering is only a numbering)
    int8_t *am_vit;                  // [S][am_nvit][2][AM_VIT]  depunctured trellis inputs: 8 x P1, P3 (am_nvit = NWIN in the window pipeline, else 1)
    int am_nvit;
    unsigned long long *am_dec;      // [am_ndec][S][8 * AM_DEC_P1 + AM_DEC_P3]  survivor decisions (one set per decode stream)
    K9Meta *am_k9meta;               // [am_ndec][S]  window pipeline: segment boundaries of the P3 frame, end states of the P1 frames
    unsigned *am_k9stats;            // [4] forward boundaries checked / re-run, traceback boundaries checked / re-walked
    AmJob *am_job;                   // [S][NWIN]
    AmCkpt *am_ckpt;                 // [S][NWIN][8]  replay: state after the block that delivered P1 PDU j of the job's frame; null unless
                                     // p1_async && l2_feedback
    float *am_ber;                   // [S][p1_slots]  window pipeline: BER of the L1 frame in each ring slot
    int8_t *am_pids_stage;           // [S][NWIN][8][240]  window pipeline: PIDS trellis inputs awaiting k_am_decode
    int *am_pids_rec;                // [S][NWIN][8]       record index of each staged PIDS frame, -1 = empty
    nrsc5hip_l2_frame *l2_ring;      // [S][p1_slots]  engine option l2_index: audio-transport index of each P1 frame slot (else null)
    nrsc5hip_l2_frame *l2_px_ring;   // [S][px_slots][2]  same for the P3 / P4 frames of the extended sidebands (else null)
    nrsc5hip_l2_frame *l2_am_ring;   // [S][p1_slots][9]  same for the 8 P1 frames + the P3 frame of each AM L1 frame slot (else null)
};

// ---- K1 -------------------------------------------------------------------------------
// cu8 -> Q15 half-band 2:1 for one chunk per stream.  iq[s] = base + s*stride, nbytes[s] each.
// what a block step of the fast streaming seam posts into pinned host memory (engine_seam.hip: harvest)
struct StreamReport { int counters[4]; long long rd; int nblocks; int nrec; BlockRecord rec[4]; unsigned seq; unsigned pad; };
// streaming seam, ONE stream: the chunk is read where the host staged it (pinned, device-visible: no copy engine, no second buffer),
// every input byte once; the workgroup that finishes last rolls the decimator history and publishes the new write position
void launch_decimate_fm_cu8_stream(const DevTables &tb, const DevBuffers &db, int s, const uint8_t *iq, unsigned nbytes, unsigned *ticket, hipStream_t st);
// streaming seam, ONE stream: the block's PIDS frame (do_pids) and then the report (k_pids_px.hip)
void launch_stream_tail(const DevTables &tb, const DevBuffers &db, int s, int first_rec, StreamReport *out, unsigned seq, int do_pids, hipStream_t st);

void launch_decimate_fm_cu8(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids,
                            const uint8_t *iq_base, long long iq_stride, const unsigned *nbytes, unsigned max_nbytes,
                            hipStream_t st);
// engine option batch_zero_copy: attach the caller's cu8 captures to freshly reset streams (no copy, no decimation)
void launch_attach_raw(const DevBuffers &db, int nstreams, const int *stream_ids, const uint8_t *iq_base, long long iq_stride,
                       const unsigned *nbytes, hipStream_t st);
void launch_append_cs16(const DevBuffers &db, int nstreams, const int *stream_ids,
                        const int16_t *iq_base, long long iq_stride, const unsigned *nsamples, unsigned max_n, hipStream_t st);

// ---- one block step for a set of streams (k_acquire.hip, k_mixfft.hip, k_sync.hip; sync_body.h, mixfft_body.h) ----
void launch_acquire(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, hipStream_t st);
void launch_prepare(const DevBuffers &db, int nstreams, const int *stream_ids, int acq_on, hipStream_t st);
// streams whose current block runs in exact-oscillator mode (StreamState::nco_mode): the reference's 69 120-step float recurrence, one lane per stream
void launch_nco_exact(const DevBuffers &db, int nstreams, const int *stream_ids, hipStream_t st);
void launch_mixfft(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, hipStream_t st, int syms_per_wg = 1, int local_prepare = 0);
size_t flow_words(int n);
void launch_flow(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int K, unsigned *flow, unsigned *err_host, int parity, int slot0, int window, hipStream_t st);
void launch_sync(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int slot, int fuse_prepare, int window, hipStream_t st, int lanes = 0, int pids_inline = 0, int do_prepare = 0, int ext_refs = 1,
                 StreamReport *report = nullptr, unsigned report_seq = 0, int report_first = 0);   // report: one-stream launch of the fast seam posts the step's report itself (k_stream_tail's job)
// replay (k_replay.hip): apply the first-header verdicts of finished deferred P1 decodes -- rewind the stream to the failed frame
void launch_rollback(const DevBuffers &db, int nstreams, const int *stream_ids, int cur_window, int min_age, hipStream_t st);
void launch_rollback_am(const DevBuffers &db, int nstreams, const int *stream_ids, int cur_window, int min_age, hipStream_t st);
// batched FIFO trim (k_trim.hip): per listed stream, move [floor, wr) to the front of its slab and set base = floor, where floor = the oldest sample the
// stream itself or a replay checkpoint with a verdict still open may read.  plan[k] (device, one per list position): what was moved and the stream's
// counters afterwards.  row_wgs: workgroups per stream for spans whose source and destination are disjoint (an overlapping span is walked by one).
// A stream must not be listed twice
struct TrimPlan { long long off, n, base, wr; };
void launch_trim(const DevBuffers &db, int nstreams, const int *stream_ids, TrimPlan *plan, int row_wgs, hipStream_t st);
// behind the block step (k_pids_px.hip): the deferred PIDS decode ...
void launch_pids_decode(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int nslots, hipStream_t st);
// ... extended sidebands: interleaver IV for streams whose block pair just completed (after k_sync), and the staged P3/P4 decodes
void launch_px_deint(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int slot, hipStream_t st);
void launch_px_decode(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int lane_id, hipStream_t st);
// a window's P1 decode: de-interleave -> forward trellis pass -> traceback + BER + descramble + first-header verdict (+ fused L2 index)
void launch_p1_deint(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int lane_id, hipStream_t st);
// segments: waves per frame of the forward pass (1..16; clamped to what the frame length allows), see viterbi_v3.h
void launch_p1_forward(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int lane_id, hipStream_t st, int segments, int warm = 2);
// parts: workgroups per frame of the traceback's first pass (k_p1_tbmap), 1..16
void launch_p1_traceback(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int lane_id, hipStream_t st, int l2_mode = 0, int parts = 4, int walk = 1);

// ---- AM path (k_am_decimate.hip, k_am.hip, k_am_decode.hip) ---------------------------------------
// cu8 -> five cascaded half-bands 32:1, any nbytes % 4 == 0 per stream (stage phases carry over)
void launch_am_decimate_cu8(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids,
                            const uint8_t *iq_base, long long iq_stride, const unsigned *nbytes, unsigned max_nbytes, hipStream_t st);
// one block step: acquire (or track) -> 2 x 32 FFT-256 -> sync_process_am -> PIDS; then this block's P1 / P3 decodes
// and, after block 7, the bit de-interleaver of the finished L1 frame
void launch_am_step(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, hipStream_t st, int l2_feedback = 0, int pipeline_parity = -1, int slot = 0,
                    int window = 0);
// in-order mode's part of a block step (called by launch_am_step): this block's P1 frame and after block 7 the P3 frame, then their L2 index
void launch_am_decode_in_order(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int l2_feedback, hipStream_t st);
// entry of the AM de-interleave tables: cell | bit << 13 | matrix << 16 | delayed << 18 | punctured << 19
constexpr unsigned AMT_DELAYED = 1u << 18, AMT_PUNCT = 1u << 19;
// window pipeline: the 8 P1 frames and the P3 frame of every L1 frame whose de-interleave happened in window `parity`
void launch_am_decode(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int lane_id, int l2_feedback, hipStream_t st,
                      int segments, int warm, int runin);
void launch_stage_first_header(const uint32_t *words, int nwords, int nframes, int am, int threads, int *ok, hipStream_t st);
void launch_viterbi_k9_frames(const int8_t *coded, int len, int nframes, unsigned g0, unsigned g1, unsigned g2,
                              unsigned long long *dec, uint32_t *out, hipStream_t st, int phases = 3,
                              K9Meta *meta = nullptr, int segments = 1, int warm = K9_WARM, int runin = K9_TB_RUNIN, unsigned *stats = nullptr);

// ---- L2 audio transport index (k_l2.hip): one workgroup per decoded frame --------------------------------------
constexpr int L2_MAX_BYTES = 18269;
struct L2Job { const uint32_t *words; int nbits; int pad; };        // packed frame (bit i at words[i / 32] bit i % 32)
void launch_l2_index(const L2Job *jobs, int njobs, nrsc5hip_l2_frame *frames, uint8_t *bytes_out, long long stride, hipStream_t st);
// engine option l2_index: index the P1 frames k_p1_traceback finished in decode window `parity` (called by launch_p1_traceback)
void launch_l2_index_window(const DevBuffers &db, int nstreams, const int *stream_ids, int parity, hipStream_t st);
// ... the P3 / P4 frames k_px_decode just finished (called by launch_px_decode), and an AM L1 frame's frames: window pipeline
// (called by launch_am_decode) or in order (called by launch_am_step: the frames k_am_viterbi delivered this step)
void launch_l2_index_px_window(const DevBuffers &db, int nstreams, const int *stream_ids, int parity, hipStream_t st);
void launch_l2_index_am_window(const DevBuffers &db, int nstreams, const int *stream_ids, int parity, hipStream_t st);
void launch_l2_index_am_step(const DevBuffers &db, int nstreams, const int *stream_ids, hipStream_t st);

// ---- arena consumers (k_psd.hip, k_sis.hip; host side: arena_consumer.h): one wave64 workgroup per listed consumer stream walks that stream's jobs and leaves
// records in a bump-allocated arena: a record header (its first word: `pos`), then `len` bytes padded to a multiple of 4
struct ArenaStream { int target; int first; int count; int pos; };  // consumer stream, its jobs [first, first + count), position in the caller's list
struct ArenaHdr { unsigned used, count, overflow, pad; };           // bytes reserved (may exceed the capacity: then overflow is set), records stored
static_assert(sizeof(ArenaStream) == 16 && sizeof(ArenaHdr) == 16, "the plan and the arena header are moved as 16-byte entries");
constexpr unsigned ARENA_FULL = 0xffffffffu;
// room for a record of `rec` bytes (one lane calls this) -> its offset, or ARENA_FULL with the overflow flag set: nothing of the record may be written then
__device__ inline unsigned arena_reserve(ArenaHdr *hdr, unsigned cap, unsigned rec)
{
    const unsigned at = atomicAdd(&hdr->used, rec);
    if (at > cap || rec > cap - at) { atomicOr(&hdr->overflow, 1u); return ARENA_FULL; }
    return at;
}

// ---- PSD transport (k_psd.hip): HDLC de-framing of the PSD spans the L2 index marks, one wave64 workgroup per stream ------------
constexpr int PSD_MAX_AAS = 8212;                                   // MAX_AAS_LEN, frame.h:5: raw bytes of one open HDLC frame
constexpr int PSD_PROGRAMS = 8;
constexpr int PSD_STATS = 9;                                        // device counters per stream: nrsc5hip_psd_stats [0..8]
struct PsdJob { int frame; int keep; int reset; int pad; };         // frame: index into frames / bytes (-1: none); keep: PDUs walked at most; reset: close all
                                                                    // eight programs of the stream before this job (frame_reset)
// a packet in the arena: PsdPacket, then `len` data bytes (what follows port and seq), padded to a multiple of 4
struct PsdPacket { uint32_t pos; uint16_t port, seq, len; uint8_t program, pad; };
struct PsdArgs {
    const ArenaStream *streams; const PsdJob *jobs; int njobs;
    const nrsc5hip_l2_frame *frames; const uint8_t *bytes; long long stride; int nframes;
    uint8_t *bufs;                   // [consumer streams][8][PSD_MAX_AAS]  frame_t.psd_buf
    int *idx;                        // [consumer streams][8]               frame_t.psd_idx, -1 = closed
    unsigned long long *stats;       // [consumer streams][PSD_STATS]
    ArenaHdr *hdr; uint8_t *arena; unsigned arena_cap;
};
void launch_psd(const PsdArgs &a, int nstreams, hipStream_t st);

// ---- SIS (k_sis.hip): pids_frame_push / sis_decode over the PIDS frames of the block records, one wave64 workgroup per stream ----
constexpr int SIS_STATS = 30;                                       // device counters per stream: nrsc5hip_sis_stats [0..29]
enum { SIS_C_FRAMES = 0, SIS_C_CRC, SIS_C_SIS, SIS_C_LLDS, SIS_C_ID0 /* .. + 15 */, SIS_C_UNKNOWN = 20, SIS_C_NOROOM, SIS_C_NC_MESSAGE, SIS_C_NC_SLOGAN,
       SIS_C_NC_ALERT, SIS_C_BAD_CHECKSUM, SIS_C_BAD_CRC7, SIS_C_BAD_CNT_LEN, SIS_C_BAD_CNT_CRC, SIS_C_EVENTS };
// an entry of a stream's list: the frame as the record holds it (bit i at w[i / 32] bit i % 32), flags bit 0: decode_reset in front of it,
// bit 1: no frame (a REC_TO_FINE record without REC_PIDS)
struct SisFrame { uint32_t w[3]; uint32_t flags; };
// an event in the arena: SisEvent, then `len` data bytes padded to a multiple of 4
struct SisEvent { uint32_t pos, entry; uint16_t kind, len; int32_t enc; int32_t v[8]; };
// pids_t (pids.h:41-96) without the pointer; floats as the signed 22-bit integers they are made from and a flag for "not NaN"
struct SisState {
    int cc, fcc;                                                    // country code: two chars, 0 = none
    uint8_t short_name[8];
    int long_seq, long_displayed;
    int lat, lon, have_lat, have_lon, altitude;
    int msg_seq, msg_priority, msg_enc, msg_len, msg_checksum, msg_displayed;
    int asd[8][3], dsd[16][3], params[13];
    int usn_enc, usn_append, usn_len, usn_displayed;
    int slogan_enc, slogan_len, slogan_displayed;
    int alert_seq, alert_enc, alert_len, alert_crc, alert_cnt_len, alert_displayed, alert_timeout;
    uint8_t long_have[8], msg_have[32], usn_have[4], slogan_have[16], alert_have[64];
    uint8_t long_name[60], usn[16], usn_final[16], slogan[96], message[192], alert[384];
};
static_assert(sizeof(SisState) % 4 == 0, "SisState is moved as words");
struct SisArgs {
    const ArenaStream *streams; const SisFrame *frames; int nentries;
    SisState *state;                 // [consumer streams]
    int nstreams;                    // consumer streams: a target outside [0, nstreams) is not walked
    unsigned long long *stats;       // [consumer streams][SIS_STATS]
    ArenaHdr *hdr; uint8_t *arena; unsigned arena_cap;
};
void sis_state_init(SisState &s);                                   // pids_init, pids.c:1052-1102 (host)
void launch_sis(const SisArgs &a, int nstreams, hipStream_t st);

// ---- data services (k_aas.hip): output_aas_push (output.c:493-896) over the packet arena k_psd leaves in device memory, one wave64 workgroup per stream ----
constexpr int AAS_SERVICES = 16, AAS_COMPONENTS = 8;                // MAX_SIG_SERVICES, MAX_SIG_COMPONENTS (output.h:13-14)
constexpr int AAS_LOT_PER_COMPONENT = 12;                           // MAX_LOT_FILES (output.h:15)
constexpr int AAS_FRAGMENT = 256, AAS_FRAGMENTS = 256;              // LOT_FRAGMENT_SIZE, MAX_LOT_FRAGMENTS
constexpr int AAS_FILE_BYTES = AAS_FRAGMENT * AAS_FRAGMENTS;        // 65 536
constexpr int AAS_NAME_MAX = 231;                                   // hdrlen is a byte: 255 - 8 - 16
constexpr int AAS_MAX_FILES = 64;                                   // file slots per stream at most: a lane each
constexpr int AAS_STATS = 26;                                       // device counters per stream: nrsc5hip_aas_stats [0..25]
enum { AAS_C_PACKETS = 0, AAS_C_PSD, AAS_C_SIG, AAS_C_SIG_PARSED, AAS_C_SIG_TRUNCATED, AAS_C_SIG_ZERO_LEN, AAS_C_SIG_EMPTY, AAS_C_UNKNOWN_PORT,
       AAS_C_BEFORE_SIG, AAS_C_NOT_IN_SIG, AAS_C_STREAM, AAS_C_PACKET, AAS_C_UNKNOWN_TYPE, AAS_C_LOT_PACKETS, AAS_C_LOT_BAD, AAS_C_LOT_SHORT_HEADER,
       AAS_C_LOT_HEADERS, AAS_C_LOT_RESETS, AAS_C_LOT_FRAGMENTS, AAS_C_LOT_DUPLICATES, AAS_C_LOT_TOO_LARGE, AAS_C_LOT_FILES, AAS_C_LOT_OVERSIZE,
       AAS_C_LRU_EVICTIONS, AAS_C_POOL_EVICTIONS, AAS_C_EVENTS };
enum { AAS_FLAG_FRAGMENTS = 1 };                                    // NRSC5HIP_AAS_FRAGMENTS
// sig_component_t / sig_service_t (output.h:60-92) without the pointers and the files; type: SIG_COMPONENT_* / SIG_SERVICE_* (0 none, 1 data, 2 audio)
struct AasComponent { uint8_t type, id, data_type, pad; uint16_t port, service_data_type; uint32_t mime; };
struct AasService { uint8_t type, pad; uint16_t number; uint32_t name_len; uint8_t name[256]; AasComponent comp[AAS_COMPONENTS]; };
struct AasStream { AasService services[AAS_SERVICES]; uint32_t lot_lru_counter, pad[3]; };
// the table as the SIG event and nrsc5hip_aas_sig carry it (include/nrsc5hip.h has the layout); out == nullptr: count only.  -> bytes, *nservices
__host__ __device__ inline unsigned aas_sig_flatten(const AasService *sv, uint8_t *out, unsigned *nservices)
{
    unsigned n = 0, ns = 0;
    auto put = [&](unsigned b) { if (out) out[n] = (uint8_t)b; n++; };
    for (; ns < (unsigned)AAS_SERVICES && sv[ns].type != 0; ns++) {                        // nrsc5_report_sig, nrsc5.c:880-934
        const AasService &s = sv[ns];
        put(s.type); put(s.number & 0xffu); put(s.number >> 8); put(s.name_len);
        for (unsigned k = 0; k < s.name_len; k++) put(s.name[k]);
        unsigned nc = 0;
        for (int j = 0; j < AAS_COMPONENTS; j++) nc += s.comp[j].type != 0;
        put(nc);
        for (int j = 0; j < AAS_COMPONENTS; j++) {
            const AasComponent &c = s.comp[j];
            if (c.type == 0) continue;
            put(c.type); put(c.id); put(c.port & 0xffu); put(c.port >> 8); put(c.service_data_type & 0xffu); put(c.service_data_type >> 8); put(c.data_type);
            put(c.mime & 0xffu); put((c.mime >> 8) & 0xffu); put((c.mime >> 16) & 0xffu); put(c.mime >> 24);
        }
    }
    *nservices = ns;
    return n;
}
// aas_file_t (output.h:47-58): owner = service * 8 + component (-1: the slot is free), local = its index in the component's lot_files[12]
struct AasFile {
    int32_t owner, local; uint32_t lot, timestamp, size, mime; int32_t expiry[5];        // tm_year, tm_mon, tm_mday, tm_hour, tm_min
    uint32_t has_name, name_len, bytes_so_far, pad[4];
    uint32_t mask[AAS_FRAGMENTS / 32];
    uint8_t name[AAS_NAME_MAX + 1];
};
static_assert(sizeof(AasComponent) == 12 && sizeof(AasStream) % 16 == 0 && sizeof(AasFile) % 16 == 0, "the states are cleared and moved as words");
// an event in the arena: AasEvent, then `len` data bytes padded to a multiple of 4 (include/nrsc5hip.h says what each kind carries)
struct AasEvent { uint32_t pos, len; uint16_t kind, port; uint32_t seq; int32_t v[8]; };
static_assert(sizeof(AasEvent) == 48, "nrsc5hip.h and abi.py state the size");
struct AasArgs {
    const ArenaStream *streams;      // the listed streams: a workgroup takes the packets whose `pos` is its stream's
    int nstreams, lot_files, flags;  // consumer streams (a target outside is not walked), file slots per stream, AAS_FLAG_*
    const ArenaHdr *in_hdr; const uint8_t *in_arena; unsigned in_cap;     // the packet arena: PsdPacket records
    AasStream *state;                // [consumer streams]
    AasFile *files;                  // [consumer streams][lot_files]
    uint8_t *data;                   // [consumer streams][lot_files][AAS_FILE_BYTES]
    unsigned long long *stats;       // [consumer streams][AAS_STATS]
    ArenaHdr *hdr; uint8_t *arena; unsigned arena_cap;
};
void launch_aas(const AasArgs &a, int nstreams, hipStream_t st);

// ---- stage-level entry points (parity tests) ---------------------------------------------------
// scratch of the stage-level K=7 decode (end lanes, chunk maps, packed soft words, segment metadata): owned by the engine that calls it
struct VitScratch { int *endlane = nullptr; int cap = 0; uint8_t *gmap = nullptr; size_t gcap = 0; int *soft = nullptr; size_t scap = 0; int *meta = nullptr; int mcap = 0; };
void vit_scratch_free(VitScratch &sc);
// -> 0, or -1: frame too long for the block-parallel traceback (viterbi3_traceback_block: at most 64 segments of TB_SEG chunks) / out of device memory
int launch_viterbi_frames(VitScratch &sc, const int8_t *coded, int len, int nframes, unsigned long long *dec, uint32_t *out, hipStream_t st, int phases = 3, int segments = 1, int *stats = nullptr, int warm = 2);
void launch_selftest(int *fail_count, hipStream_t st);
// one function of fastmath.h (fn: NRSC5HIP_MATH_*) on n elements of device memory; -> 0, or -1: unknown fn / n < 1
int launch_stage_math(int fn, const void *a, const void *b, long long n, void *out0, void *out1, hipStream_t st);
void launch_fft2048(const DevTables &tb, const float2 *in, float2 *out, int nffts, hipStream_t st, int form = 1);   // form 32: the 256-lane FFT
// the fused half-band's forms on a raw cu8 capture in device memory (nrsc5hip_stage_halfband_raw; the caller has checked that every sample read lies
// inside it).  Symbol forms (k_mixfft.hip): lanes = 128 or 256, nsyms workgroups, out[nsyms][2160]; pc = four floats {1, 1.5 * 2^-24, 2^-126, 0.5}
// and probe[nsyms][lanes][4] for the rounding-mode probes, both null for none.  Acquisition form (k_acquire.hip): n samples from a0.
void launch_stage_halfband_sym(const DevTables &tb, int lanes, const uint8_t *raw, long long a0, int nsyms, c16 *out, const float *pc, uint32_t *probe, hipStream_t st);
void launch_stage_halfband_acq(const DevTables &tb, const uint8_t *raw, long long a0, long long n, c16 *out, hipStream_t st);
// the FEC stage hooks (nrsc5hip_stage_pids / _am_deinterleave / _am_epilogue; the others need the production launchers above only).
// PIDS gather + depuncture of block bc of the soft-bit matrices pm through tb.pids_gather into stage[240] (k_pids_px.hip: sync_body.h's two lines restated)
void launch_stage_pids_gather(const DevTables &tb, const int8_t *pm, int bc, int8_t *stage, hipStream_t st);
// k_am_block alone on stream 0 (k_am.hip; launch_am_step's first launch): <256> in order (pipeline 0), <512> as the window pipeline launches it (pipeline 1: window parity 0,
// slot 0); dump_x [NSYM * AM_FFT] / dump_mult [4 * AM_PW] non-null: the instantiation that copies the tile behind the sideband combine and the equaliser taps out
void launch_stage_am_block(const DevTables &tb, const DevBuffers &db, int pipeline, float2 *dump_x, float2 *dump_mult, hipStream_t st);
// k_am_interleave alone (k_am.hip; launch_am_step's last launch)
void launch_am_interleave(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int window, hipStream_t st);
// am_p3_epilogue (k_am_decode.hip) on the frame am_decode_frame(vit, slot, ., role, psmi) describes, one workgroup of `threads`: vit [2][AM_VIT]
// trellis inputs, slot [P1_WORDS] the packed decoded bits (descrambled in place), *err the count
void launch_stage_am_epilogue(const DevTables &tb, const int8_t *vit, uint32_t *slot, int role, int psmi, int threads, int *err, hipStream_t st);

}  // namespace nrsc5
