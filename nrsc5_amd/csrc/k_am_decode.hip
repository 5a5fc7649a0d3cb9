// AM frame decode for gfx950: what turns the trellis inputs of an L1 frame (k_am_interleave, k_am.hip) into delivered frames.
// Replaces decode_process_p1_p3_am with nrsc5_conv_decode_e1 / _e2_e3, bit_errors and descramble (decode.c:234-294,507-554):
//   in order, on the main stream, one block's frames per step                       -> k_am_viterbi
//   window pipeline, the nine frames of an L1 frame at once on a decode stream      -> k_am_decode_fwd / _fix / _tb / _finish
// and holds the stage-level K=9 entry points of the parity tests.  The trellis itself: viterbi_k9.h.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "wave_ops.h"
#include "l2_header.h"
#include "viterbi_k9.h"

namespace nrsc5 {

// ---- one frame of an AM L1 frame: where it lies and which code it carries ---------------------------------------------
// (decode_process_p1_p3_am, decode.c:507-554: the P1 frames and an MA3 P3 frame are E1, an MA1 P3 frame is E2)
struct AmDecodeFrame { const int8_t *in; uint32_t *out; unsigned long long *dec; int len; unsigned g0, g1, g2, pmask; int plen; };

// role 0..7: the P1 frame of that block, 8: the P3 frame.  vit: the L1 frame's trellis inputs, slot: its ring slot, dec: the
// caller's decision scratch (8 x AM_DEC_P1 + AM_DEC_P3)
__device__ inline AmDecodeFrame am_decode_frame(const int8_t *vit, uint32_t *slot, unsigned long long *dec, int role, int psmi)
{
    AmDecodeFrame f;
    const bool e1 = role < 8 || psmi == AM_MA3;
    if (role < 8) {
        f.in = vit + (size_t)role * AM_P1_LEN * 3; f.out = slot + role * AM_P1_WORDS; f.dec = dec + (size_t)role * AM_DEC_P1;
        f.len = AM_P1_LEN;
    } else {
        f.in = vit + AM_VIT; f.out = slot + AM_P3_WORD0; f.dec = dec + (size_t)8 * AM_DEC_P1;
        f.len = psmi == AM_MA3 ? AM_P3_LEN_MA3 : AM_P3_LEN_MA1;
    }
    f.g0 = e1 ? GEN_E1_0 : GEN_E2_0; f.g1 = e1 ? GEN_E1_1 : GEN_E2_1; f.g2 = e1 ? GEN_E1_2 : GEN_E2_2;
    f.pmask = e1 ? PUNCT_E1 : PUNCT_E2; f.plen = e1 ? 15 : 6;
    return f;
}

// out ^= the scrambler stream, in place; the bits of the last word beyond the frame are cleared (a P1 frame's last word holds 6)
__device__ inline void am_descramble(uint32_t *out, const uint32_t *scr, int len)
{
    const int words = (len + 31) / 32;
    const uint32_t tailmask = (len & 31) ? (1u << (len & 31)) - 1u : 0xffffffffu;
    for (int w = threadIdx.x; w < words; w += blockDim.x) out[w] = (out[w] ^ scr[w]) & (w == words - 1 ? tailmask : 0xffffffffu);
}

// the frame's (still scrambled) bits are in f.out and visible to the workgroup: bit errors against the trellis inputs, descramble
__device__ inline int am_p3_epilogue(const DevTables &tb, const AmDecodeFrame &f, int *red)
{
    const int err = am_bit_errors(f.in, f.out, f.len, f.g0, f.g1, f.g2, f.pmask, f.plen, red);
    am_descramble(f.out, tb.scr_p1, f.len);
    return err;
}

// Out of line on purpose, as the compiler had it while the check had two callers in one unit: inlined, its Reed-Solomon decode takes
// k_am_viterbi to 65 VGPRs and from 8 waves per SIMD to 7
__device__ __attribute__((noinline)) bool am_first_header_ok(const uint32_t *out, L2Smem &l2) { return l2_first_header_ok_am_block(out, l2); }

// ... and for a P1 frame, on request, the verdict on its first L2 header (frame.c:535-540 for the 466-byte AM PDU)
__device__ inline int am_p1_epilogue(const DevTables &tb, const AmDecodeFrame &f, K9WSmem &k9, int *red, int l2_feedback, bool &hdr_ok)
{
    const int err = am_p3_epilogue(tb, f, red);
    __threadfence_block();
    __syncthreads();
    static_assert(sizeof(L2Smem) <= sizeof(K9WSmem), "L2 scratch aliases the trellis scratch");
    L2Smem &l2 = *(L2Smem *)&k9;                               // the trellis scratch is dead by now
    hdr_ok = l2_feedback ? am_first_header_ok(f.out, l2) : true;
    return err;
}

__device__ inline int am_whole_p3(const DevTables &tb, const AmDecodeFrame &f, K9WSmem &k9, int *red)
{
    viterbi_k9_wave(f.in, f.len, f.g0, f.g1, f.g2, f.dec, f.out, k9);
    return am_p3_epilogue(tb, f, red);
}

// ---- in order: this block's P1 frame, and after block 7 the P3 frame -------------------------------------------------
__global__ __launch_bounds__(64) void k_am_viterbi(DevTables tb, DevBuffers db, const int *ids, int l2_feedback)
{
    const int s = stream_of(ids, blockIdx.y);
    const StreamState &st = db.state[s];
    AmStream &am = db.am[s];
    if (!st.active || am.dec_bc < 0 || am.am_diversity_wait != 0) return;      // block-uniform
    const int role = blockIdx.x, bc = am.dec_bc;                                 // 0: P1, 1: P3 (in-order mode)
    if (role == 1 && (bc != 7 || am.dec_rdbi)) return;
    __shared__ K9WSmem k9;
    __shared__ int red[4];
    // one set of trellis inputs and one of decision scratch per stream
    const int8_t *vit = db.am_vit + (size_t)s * db.am_nvit * 2 * AM_VIT;
    uint32_t *slot = db.p1_ring + ((size_t)s * db.p1_slots + am.frame_slot) * P1_WORDS;
    unsigned long long *dec = db.am_dec + (size_t)s * (size_t)(8 * AM_DEC_P1 + AM_DEC_P3);
    BlockRecord &rec = db.records[(size_t)s * db.rec_cap + am.dec_record];
    // The whole-frame wave is compiled once per kind of frame (P1, P3 of MA3, P3 of MA1), each with its length and code as constants:
    // with them a variable, the P3 wave -- the longest launch of the in-order pass -- measured 10 % slower.  (bc & 7: bc is 0..7)
    if (role == 0) {
        const AmDecodeFrame f = am_decode_frame(vit, slot, dec, bc & 7, am.dec_psmi);
        viterbi_k9_wave(f.in, f.len, f.g0, f.g1, f.g2, f.dec, f.out, k9);
        bool hdr_ok;
        const int err = am_p1_epilogue(tb, f, k9, red, l2_feedback, hdr_ok);
        if (threadIdx.x == 0) {
            atomicAdd(&am.am_errors, (unsigned)err);
            atomicOr(&rec.flags, (uint32_t)REC_P1);
            rec.p1_slot = am.frame_slot;
            StreamState &stw = db.state[s];
            if (!hdr_ok && stw.sync_state == SYNC_FINE) { stw.sync_state = SYNC_NONE; rec.state_after = SYNC_NONE; atomicOr(&rec.flags, (uint32_t)REC_LOST_SYNC); }
        }
    } else {
        int err;
        if (am.dec_psmi == AM_MA3) err = am_whole_p3(tb, am_decode_frame(vit, slot, dec, 8, AM_MA3), k9, red);
        else err = am_whole_p3(tb, am_decode_frame(vit, slot, dec, 8, am.dec_psmi), k9, red);          // (known not to be MA3 here)
        if (threadIdx.x == 0) {
            atomicAdd(&am.am_errors, (unsigned)err);
            atomicOr(&rec.flags, (uint32_t)REC_P3);
        }
    }
}

void launch_am_decode_in_order(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int l2_feedback, hipStream_t st)
{
    hipLaunchKernelGGL(k_am_viterbi, dim3(2, nstreams), dim3(64), 0, st, tb, db, stream_ids, l2_feedback);
    if (db.l2_am_ring) launch_l2_index_am_step(db, nstreams, stream_ids, st);
}

// ---- window pipeline: all nine frames of an L1 frame decode concurrently on a decode stream ---------------------------
// Four launches (the P3 frame is 6.4 / 8 times a P1 frame: as ONE wave it kept the launch -- and a decode stream -- alive for
// 4-5 ms after the P1 waves had gone; in K9_GMAX segment waves every wave of the launch is about one P1 frame long):
//   k_am_decode_fwd     forward pass: 8 P1 waves, G P3 segment waves, 8 PIDS frames (whole: 144 steps)
//   k_am_decode_fix     P3: segment boundaries checked / re-run, end state
//   k_am_decode_tb      traceback: P1 frames whole + BER, descramble, first-header verdict; P3 in G segment waves
//   k_am_decode_finish  P3: traceback boundaries checked / re-walked, BER, descramble; frame accounting
// one set of trellis inputs per window in flight, one of decision scratch per decode stream
__device__ inline AmDecodeFrame am_window_frame(const DevBuffers &db, const AmJob &job, int s, int parity, int lane_id, int role)
{
    return am_decode_frame(db.am_vit + ((size_t)s * db.am_nvit + parity) * 2 * AM_VIT, db.p1_ring + ((size_t)s * db.p1_slots + job.slot) * P1_WORDS,
                           db.am_dec + ((size_t)lane_id * db.nstreams_alloc + s) * (size_t)(8 * AM_DEC_P1 + AM_DEC_P3), role, job.psmi);
}

// the frame is decoded: count it, and the last of the L1 frame's decodes closes the job (nrsc5_report_ber's value, decode.c:545)
__device__ inline void am_decode_account(const DevBuffers &db, AmJob &job, int s, int err)
{
    if (threadIdx.x != 0) return;
    atomicAdd(&job.errors, (unsigned)err);
    __threadfence();
    const int expected = job.rdbi ? 8 : 9;
    if (atomicAdd(&job.done, 1) == expected - 1) {
        db.am_ber[(size_t)s * db.p1_slots + job.slot] = (float)atomicAdd(&job.errors, 0u) / (float)am_frame_coded_bits(job.psmi, job.rdbi);
        job.pad = db.l2_am_ring ? (job.rdbi ? 0xff : 0x1ff) : 0;      // frames k_l2_index_am_window owes their index
        job.valid = 0;
    }
}

__global__ __launch_bounds__(64) void k_am_decode_fwd(DevTables tb, DevBuffers db, const int *ids, int parity, int lane_id, int G, int warm)
{
    const int s = stream_of(ids, blockIdx.y), role = blockIdx.x;           // 0..7: P1 frame of that block, 8..8+G-1: P3 segment, then 8 PIDS frames
    __shared__ K9WSmem k9;
    if (role >= 8 + G) {
        // decode_process_pids_am's trellis (decode.c:502-504) for the block processed in step `pb` of this window
        const int pb = role - 8 - G;
        int *recp = db.am_pids_rec + ((size_t)s * NWIN + parity) * 8 + pb;
        const int r = *recp;
        if (r < 0) return;                                                 // wave-uniform
        __shared__ uint32_t pout[4];
        const int8_t *stage = db.am_pids_stage + (((size_t)s * NWIN + parity) * 8 + pb) * (3 * PIDS_LEN);
        unsigned long long *pdec = db.am_dec + ((size_t)lane_id * db.nstreams_alloc + s) * (size_t)(8 * AM_DEC_P1 + AM_DEC_P3)
                                 + (size_t)8 * AM_DEC_P1 + AM_DEC_P3 - (size_t)(9 - pb) * 4 * (PIDS_LEN + 64);   // tail of the P3 scratch: its frame is shorter than AM_P3_LEN_MA3 + 64 only by the slack reserved here
        viterbi_k9_wave(stage, PIDS_LEN, GEN_E2_0, GEN_E2_1, GEN_E2_2, pdec, pout, k9);
        if (threadIdx.x == 0) {
            BlockRecord &rec = db.records[(size_t)s * db.rec_cap + r];
            const uint32_t p[3] = { pout[0] ^ tb.scr_pids[0], pout[1] ^ tb.scr_pids[1], (pout[2] ^ tb.scr_pids[2]) & 0xffffu };
            rec.pids[0] = p[0]; rec.pids[1] = p[1]; rec.pids[2] = p[2];
            if (pids_crc_ok(p)) atomicOr(&rec.flags, (uint32_t)REC_PIDS_CRC);
            *recp = -1;
        }
        return;
    }
    const AmJob &job = db.am_job[(size_t)s * NWIN + parity];
    if (!job.valid) return;                                                // wave-uniform
    if (role >= 8 && job.rdbi) return;
    K9Meta &meta = db.am_k9meta[(size_t)lane_id * db.nstreams_alloc + s];
    const AmDecodeFrame f = am_window_frame(db, job, s, parity, lane_id, role);
    if (role < 8) {
        const int lane = threadIdx.x;
        const K9Signs sg = k9_signs(lane, f.g0, f.g1, f.g2);
        for (int k = 0; k < 4; k++) k9.metric[0][4 * lane + k] = 0;
        WAVE_LDS_SYNC();
        const int cur = k9_forward_chunks(f.in, f.len, sg, f.dec, k9, 0, k9_chunks(f.len), 0, nullptr);
        const unsigned end = k9_end_state(*(const int4 *)&k9.metric[cur][4 * lane]);
        if (lane == 0) meta.p1_end[role] = end;
    } else {
        k9_forward_segment(f.in, f.len, f.g0, f.g1, f.g2, f.dec, meta, k9, role - 8, G, warm);
    }
}

__global__ __launch_bounds__(64) void k_am_decode_fix(DevBuffers db, const int *ids, int parity, int lane_id, int G)
{
    const int s = stream_of(ids, blockIdx.x);
    const AmJob &job = db.am_job[(size_t)s * NWIN + parity];
    if (!job.valid || job.rdbi) return;                                    // wave-uniform
    __shared__ K9WSmem k9;
    K9Meta &meta = db.am_k9meta[(size_t)lane_id * db.nstreams_alloc + s];
    const AmDecodeFrame f = am_window_frame(db, job, s, parity, lane_id, 8);
    const unsigned end = k9_forward_fix(f.in, f.len, f.g0, f.g1, f.g2, f.dec, meta, k9, G, db.am_k9stats);
    if (threadIdx.x == 0) meta.end_state = end;
}

__global__ __launch_bounds__(64) void k_am_decode_tb(DevTables tb, DevBuffers db, const int *ids, int parity, int lane_id, int G, int runin, int l2_feedback)
{
    const int s = stream_of(ids, blockIdx.y), role = blockIdx.x;           // 0..7: P1 frame of that block, 8..8+G-1: P3 segment
    AmJob &job = db.am_job[(size_t)s * NWIN + parity];
    if (!job.valid) return;                                                // wave-uniform
    if (role >= 8 && job.rdbi) return;
    __shared__ K9WSmem k9;
    __shared__ int red[4];
    K9Meta &meta = db.am_k9meta[(size_t)lane_id * db.nstreams_alloc + s];
    const AmDecodeFrame f = am_window_frame(db, job, s, parity, lane_id, role);
    if (role >= 8) { k9_traceback_segment(f.dec, f.len, meta, k9, f.out, role - 8, G, runin); return; }
    unsigned arrive = 0;
    const int ntb = (k9_pairs(f.len) + 31) >> 5;
    k9_traceback_chunks(f.dec, f.len, k9, (unsigned)wave_uniform((int)meta.p1_end[role]), ntb, 0, ntb, f.out, arrive);
    __threadfence_block();
    __syncthreads();
    bool ok;
    const int err = am_p1_epilogue(tb, f, k9, red, l2_feedback, ok);
    if (l2_feedback && threadIdx.x == 0) { __threadfence(); atomicExch(&job.verdict[role], ok ? 1 : 2); }   // file the verdict for the block that delivers this PDU
    am_decode_account(db, job, s, err);
}

__global__ __launch_bounds__(64) void k_am_decode_finish(DevTables tb, DevBuffers db, const int *ids, int parity, int lane_id, int G)
{
    const int s = stream_of(ids, blockIdx.x);
    AmJob &job = db.am_job[(size_t)s * NWIN + parity];
    if (!job.valid || job.rdbi) return;                                    // wave-uniform
    __shared__ K9WSmem k9;
    __shared__ int red[4];
    K9Meta &meta = db.am_k9meta[(size_t)lane_id * db.nstreams_alloc + s];
    const AmDecodeFrame f = am_window_frame(db, job, s, parity, lane_id, 8);
    k9_traceback_fix(f.dec, f.len, meta, k9, f.out, G, db.am_k9stats);
    am_decode_account(db, job, s, am_p3_epilogue(tb, f, red));
}

void launch_am_decode(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int lane_id, int l2_feedback, hipStream_t st,
                      int segments, int warm, int runin)
{
    const int G = segments < 1 ? 1 : segments > K9_GMAX ? K9_GMAX : segments;
    hipLaunchKernelGGL(k_am_decode_fwd, dim3(8 + G + 8, nstreams), dim3(64), 0, st, tb, db, stream_ids, parity, lane_id, G, warm);
    hipLaunchKernelGGL(k_am_decode_fix, dim3(nstreams), dim3(64), 0, st, db, stream_ids, parity, lane_id, G);
    hipLaunchKernelGGL(k_am_decode_tb, dim3(8 + G, nstreams), dim3(64), 0, st, tb, db, stream_ids, parity, lane_id, G, runin, l2_feedback);
    hipLaunchKernelGGL(k_am_decode_finish, dim3(nstreams), dim3(64), 0, st, tb, db, stream_ids, parity, lane_id, G);
    if (db.l2_am_ring) launch_l2_index_am_window(db, nstreams, stream_ids, parity, st);
}

// ---- stage-level entry (nrsc5hip_stage_am_epilogue): the frame epilogue alone, on a frame laid out as am_decode_frame expects it ----
template <int NT> __global__ __launch_bounds__(NT) void k_stage_am_epilogue(DevTables tb, const int8_t *vit, uint32_t *slot, int role, int psmi, int *err)
{
    __shared__ int red[4];
    const AmDecodeFrame f = am_decode_frame(vit, slot, nullptr, role, psmi);
    const int n = am_p3_epilogue(tb, f, red);
    if (threadIdx.x == 0) *err = n;
}
void launch_stage_am_epilogue(const DevTables &tb, const int8_t *vit, uint32_t *slot, int role, int psmi, int threads, int *err, hipStream_t st)
{
    if (threads == 256) hipLaunchKernelGGL(k_stage_am_epilogue<256>, dim3(1), dim3(256), 0, st, tb, vit, slot, role, psmi, err);
    else hipLaunchKernelGGL(k_stage_am_epilogue<64>, dim3(1), dim3(64), 0, st, tb, vit, slot, role, psmi, err);
}

// ---- stage-level entry: decode `nframes` independent K=9 frames (parity tests) ------------------------------------
__global__ __launch_bounds__(256) void k_viterbi_k9_frames(const int8_t *coded, int len, unsigned g0, unsigned g1, unsigned g2,
                                                           unsigned long long *dec, uint32_t *out)
{
    __shared__ K9Smem k9;
    const int f = blockIdx.x;
    viterbi_k9_block(coded + (size_t)f * 3 * len, len, g0, g1, g2, dec + (size_t)f * 4 * (len + 64), out + (size_t)f * ((len + 31) / 32), k9);
}
__global__ __launch_bounds__(64) void k_viterbi_k9_frames_wave(const int8_t *coded, int len, unsigned g0, unsigned g1, unsigned g2,
                                                               unsigned long long *dec, uint32_t *out, int phases)
{
    __shared__ K9WSmem k9;
    const int f = blockIdx.x;
    viterbi_k9_wave(coded + (size_t)f * 3 * len, len, g0, g1, g2, dec + (size_t)f * 4 * (len + 64), out + (size_t)f * ((len + 31) / 32), k9, phases);
}
// the segment-wave form, one launch per stage (what k_am_decode_* do for the P3 frame)
__global__ __launch_bounds__(64) void k_k9seg_fwd(const int8_t *coded, int len, unsigned g0, unsigned g1, unsigned g2, unsigned long long *dec, K9Meta *meta, int G, int warm)
{
    __shared__ K9WSmem k9;
    const int f = blockIdx.y;
    k9_forward_segment(coded + (size_t)f * 3 * len, len, g0, g1, g2, dec + (size_t)f * 4 * (len + 64), meta[f], k9, (int)blockIdx.x, G, warm);
}
__global__ __launch_bounds__(64) void k_k9seg_fix(const int8_t *coded, int len, unsigned g0, unsigned g1, unsigned g2, unsigned long long *dec, K9Meta *meta, int G, unsigned *stats)
{
    __shared__ K9WSmem k9;
    const int f = blockIdx.x;
    const unsigned end = k9_forward_fix(coded + (size_t)f * 3 * len, len, g0, g1, g2, dec + (size_t)f * 4 * (len + 64), meta[f], k9, G, stats);
    if (threadIdx.x == 0) meta[f].end_state = end;
}
__global__ __launch_bounds__(64) void k_k9seg_tb(const unsigned long long *dec, int len, K9Meta *meta, uint32_t *out, int G, int runin)
{
    __shared__ K9WSmem k9;
    const int f = blockIdx.y;
    k9_traceback_segment(dec + (size_t)f * 4 * (len + 64), len, meta[f], k9, out + (size_t)f * ((len + 31) / 32), (int)blockIdx.x, G, runin);
}
__global__ __launch_bounds__(64) void k_k9seg_finish(const unsigned long long *dec, int len, K9Meta *meta, uint32_t *out, int G, unsigned *stats)
{
    __shared__ K9WSmem k9;
    const int f = blockIdx.x;
    k9_traceback_fix(dec + (size_t)f * 4 * (len + 64), len, meta[f], k9, out + (size_t)f * ((len + 31) / 32), G, stats);
}

void launch_viterbi_k9_frames(const int8_t *coded, int len, int nframes, unsigned g0, unsigned g1, unsigned g2,
                              unsigned long long *dec, uint32_t *out, hipStream_t st, int phases, K9Meta *meta, int segments, int warm, int runin, unsigned *stats)
{
    // frames longer than a PIDS frame take the production wave form (in segment waves when `meta` is given); 80-bit frames the
    // 256-work-item form
    if (len > 80 && meta) {
        const int G = segments < 1 ? 1 : segments > K9_GMAX ? K9_GMAX : segments;
        if (phases & 1) {
            hipLaunchKernelGGL(k_k9seg_fwd, dim3(G, nframes), dim3(64), 0, st, coded, len, g0, g1, g2, dec, meta, G, warm);
            hipLaunchKernelGGL(k_k9seg_fix, dim3(nframes), dim3(64), 0, st, coded, len, g0, g1, g2, dec, meta, G, stats);
        }
        if (phases & 2) {
            hipLaunchKernelGGL(k_k9seg_tb, dim3(G, nframes), dim3(64), 0, st, dec, len, meta, out, G, runin);
            hipLaunchKernelGGL(k_k9seg_finish, dim3(nframes), dim3(64), 0, st, dec, len, meta, out, G, stats);
        }
    }
    else if (len > 80) hipLaunchKernelGGL(k_viterbi_k9_frames_wave, dim3(nframes), dim3(64), 0, st, coded, len, g0, g1, g2, dec, out, phases);
    else hipLaunchKernelGGL(k_viterbi_k9_frames, dim3(nframes), dim3(256), 0, st, coded, len, g0, g1, g2, dec, out);
}

}  // namespace nrsc5
