// PIDS part of K6/K7/K8 and the extended sidebands for gfx950 -- the small kernels behind the block step (k_sync.hip): the deferred PIDS decode
// (decode_process_pids, decode.c:463-472), the streaming seam's k_stream_tail (that decode + the step's report), interleaver IV of a completed block pair
// (decode.c:344-376) and the staged P3 / P4 decodes (decode.c:407-409,430-432).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "wave_ops.h"
#include "viterbi_wave.h"
#include "l2_header.h"

namespace nrsc5 {

// ---- deferred PIDS decode: one wave per (slot, stream) with a staged frame -----------------------------------
// called by the 64 lanes of one wave; LDS scratch from the caller
__device__ __forceinline__ void pids_decode_wave(const DevTables &tb, const DevBuffers &db, int s, int parity, int slot, int8_t *coded, unsigned long long *dec, uint32_t *out)
{
    int *recp = db.pids_rec + ((size_t)s * NWIN + parity) * 16 + slot;
    const int r = *recp;
    if (r < 0) return;                                         // wave-uniform
    const int8_t *stage = db.pids_stage + (((size_t)s * NWIN + parity) * 16 + slot) * (3 * PIDS_LEN);
    const int lane = threadIdx.x & 63;
    static_assert((3 * PIDS_LEN) % 4 == 0 && 3 * PIDS_LEN / 4 <= 64, "the staged frame is one dword per lane");
    if (lane < 3 * PIDS_LEN / 4) ((uint32_t *)coded)[lane] = ((const uint32_t *)stage)[lane];
    WAVE_LDS_SYNC();
    viterbi_k7_wave_compact<PIDS_LEN>(coded, dec, out);        // the rotating-layout trellis in its compact form, inlined with the frame length a constant
    WAVE_LDS_SYNC();
    // (the CRC runs over a local copy: handed the record itself it re-read the words from global memory for each of its 80 bits -- ~17 us of the 22.7 us this decode used to
    //  take; round 6: by the whole wave, pids_crc_ok_wave)
    const uint32_t p[3] = { out[0] ^ tb.scr_pids[0], out[1] ^ tb.scr_pids[1], (out[2] ^ tb.scr_pids[2]) & 0xffffu };   // descramble (decode.c:470)
    const bool crc_ok = pids_crc_ok_wave(p);
    if (lane == 0) {
        BlockRecord &rec = db.records[(size_t)s * db.rec_cap + r];
        rec.pids[0] = p[0]; rec.pids[1] = p[1]; rec.pids[2] = p[2];
        if (crc_ok) atomicOr(&rec.flags, (uint32_t)REC_PIDS_CRC);
        *recp = -1;
    }
}

__global__ __launch_bounds__(64) void k_pids_decode(DevTables tb, DevBuffers db, const int *ids, int parity)
{
    const int s = stream_of(ids, blockIdx.y), slot = blockIdx.x;
    __shared__ __attribute__((aligned(16))) int8_t coded[3 * PIDS_LEN];
    __shared__ unsigned long long dec[PIDS_LEN + 64];
    __shared__ uint32_t out[4];
    pids_decode_wave(tb, db, s, parity, slot, coded, dec, out);
}

// Streaming seam: the tail of ONE stream's block step in one launch -- the block's PIDS frame (in-order mode files it in slot 0 of
// window slot 0), then what the host needs into pinned host memory: the step's counters, the FIFO read position and the records
// [first_rec, nblocks) (a block's record is final when its step ends) and, last of all, the sequence number the host is waiting
// for.  Leaves the step counters at zero for the next step.  (As two launches, k_pids_decode + the report: one more ~4 us dispatch
// on a chain the host waits for.)
__global__ __launch_bounds__(64) void k_stream_tail(DevTables tb, DevBuffers db, int s, int first_rec, StreamReport *out, unsigned seq, int do_pids)
{
    __shared__ __attribute__((aligned(16))) int8_t coded[3 * PIDS_LEN];
    __shared__ unsigned long long dec[PIDS_LEN + 64];
    __shared__ uint32_t bits[4];
    const int t = threadIdx.x;
    if (do_pids) pids_decode_wave(tb, db, s, 0, 0, coded, dec, bits);       // one wave: the whole workgroup
    __threadfence();
    __syncthreads();
    const StreamState &st = db.state[s];
    const int n = min(max(st.nblocks - first_rec, 0), 4);
    constexpr int RW = sizeof(BlockRecord) / 4;
    for (int q = t; q < n * RW; q += 64) {
        const int k = q / RW, w = q % RW;
        ((uint32_t *)&out->rec[k])[w] = ((const uint32_t *)&db.records[(size_t)s * db.rec_cap + ((first_rec + k) % db.rec_cap)])[w];
    }
    if (t < 4) { out->counters[t] = db.counters[t]; db.counters[t] = 0; }
    if (t == 0) { out->rd = st.rd; out->nblocks = st.nblocks; out->nrec = n; }
    __threadfence_system();
    __syncthreads();
    if (t == 0) { *(volatile unsigned *)&out->seq = seq; __threadfence_system(); }
}

void launch_stream_tail(const DevTables &tb, const DevBuffers &db, int s, int first_rec, StreamReport *out, unsigned seq, int do_pids, hipStream_t st)
{
    hipLaunchKernelGGL(k_stream_tail, dim3(1), dim3(64), 0, st, tb, db, s, first_rec, out, seq, do_pids);
}

void launch_pids_decode(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int nslots, hipStream_t st)
{
    hipLaunchKernelGGL(k_pids_decode, dim3(nslots, nstreams), dim3(64), 0, st, tb, db, stream_ids, parity);
}

// ---- stage-level entry (nrsc5hip_stage_pids): the gather + depuncture k_sync runs in front of k_pids_decode -- sync_body.h's two lines restated
// over the production table (factoring them out of the block step would touch k_sync / k_flow; the table is what the test is about), the soft
// bits read from the frame's matrices in global memory
__global__ __launch_bounds__(256) void k_stage_pids_gather(DevTables tb, const int8_t *pm, int bc, int8_t *stage)
{
    const int tid = threadIdx.x;
    for (int n = tid; n < PIDS_CODED; n += 256) stage[n + n / 5] = pm[(size_t)bc * PM_BLOCK + (int)tb.pids_gather[bc * PIDS_CODED + n]];
    for (int n = tid; n < PIDS_CODED / 5; n += 256) stage[6 * n + 5] = 0;
}
void launch_stage_pids_gather(const DevTables &tb, const int8_t *pm, int bc, int8_t *stage, hipStream_t st)
{
    hipLaunchKernelGGL(k_stage_pids_gather, dim3(1), dim3(256), 0, st, tb, pm, bc, stage);
}

// ---- extended sidebands: interleaver IV (decode.c:344-376) for a completed block pair ----------------------------
// The interleaver is convolutional: the bit read at position i of a pair was written delay[i] positions earlier
// (1..N, N = 32 blocks), either earlier in this pair (take it from the pair buffer) or in the memory.  All reads of a
// pair happen before its writes, as in the reference's read-then-write loop, by splitting the pass at a barrier.
__global__ __launch_bounds__(1024) void k_px_deint(DevTables tb, DevBuffers db, const int *ids, int parity, int slot)
{
    const int s = stream_of(ids, blockIdx.y), ch = blockIdx.x;
    StreamState &st = db.state[s];
    const int len = st.px_go;                                  // block-uniform
    if (len == 0 || ch >= st.px_nch) return;
    const int N = 32 * len, tid = threadIdx.x;
    int I = st.px_pos, ready = st.px_ready;
    if (I == N) { I = 0; ready = 1; }
    const uint32_t *delay = len == PX_MAX ? tb.px_delay_wide : tb.px_delay_narrow;
    int8_t *mem = db.px_mem + ((size_t)s * 2 + ch) * PX_MEM;
    const int8_t *pair = db.px_pair + ((size_t)s * 2 + ch) * 2 * PX_MAX;
    int8_t *stage = db.px_stage + ((((size_t)s * NWIN + parity) * 8 + (slot >> 1)) * 2 + ch) * PX_DEPUNCT;
    int8_t vals[2 * PX_MAX / 1024];
#pragma unroll
    for (int r = 0; r < 2 * PX_MAX / 1024; r++) {
        const int i = tid + 1024 * r;
        vals[r] = 0;
        if (i < 2 * len) {
            const int d = (int)delay[i];
            vals[r] = d <= i ? pair[i - d] : mem[(I + i - d + N) % N];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2 * PX_MAX / 1024; r++) {
        const int i = tid + 1024 * r;
        if (i < 2 * len) {
            mem[I + i] = pair[i];
            const int o = (i >> 2) * 6 + (i & 3) + ((i & 3) >= 1) + ((i & 3) >= 3);   // kept positions 0, 2, 3, 5 of [1,0,1,1,0,1]
            stage[o] = vals[r];
            if ((i & 3) == 0) { stage[o + 1] = 0; stage[o + 4] = 0; }
        }
    }
    if (tid == 0) {
        PxJob &job = db.px_job[(((size_t)s * NWIN + parity) * 8 + (slot >> 1)) * 2 + ch];
        job.rec = ready ? st.px_record : -1; job.slot = st.px_slot; job.len = len; job.pad = 0;
    }
}

// both channels read px_pos / px_ready above; advance them once both are done
__global__ void k_px_commit(DevBuffers db, const int *ids, int nstreams)
{
    const int sidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (sidx >= nstreams) return;
    StreamState &st = db.state[stream_of(ids, sidx)];
    if (st.px_go == 0) return;
    const int N = 32 * st.px_go;
    if (st.px_pos == N) { st.px_pos = 0; st.px_ready = 1; }
    st.px_pos += 2 * st.px_go;
    st.px_go = 0;
}

void launch_px_deint(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int slot, hipStream_t st)
{
    hipLaunchKernelGGL(k_px_deint, dim3(2, nstreams), dim3(1024), 0, st, tb, db, stream_ids, parity, slot);
    hipLaunchKernelGGL(k_px_commit, dim3((nstreams + 63) / 64), dim3(64), 0, st, db, stream_ids, nstreams);
}

// ---- staged P3 / P4 frames: K=7 Viterbi (nrsc5_conv_decode_p3_p4), descramble (decode.c:407-409,430-432) --------
__global__ __launch_bounds__(64) void k_px_decode(DevTables tb, DevBuffers db, const int *ids, int parity, int lane_id)
{
    const int s = stream_of(ids, blockIdx.y), j = blockIdx.x;   // j = pair slot * 2 + channel
    PxJob &job = db.px_job[((size_t)s * NWIN + parity) * 16 + j];
    if (job.rec < 0) return;                                   // wave-uniform
    const int len = job.len, ch = j & 1;
    const int8_t *coded = db.px_stage + (((size_t)s * NWIN + parity) * 16 + j) * PX_DEPUNCT;
    unsigned long long *dec = db.px_dec + (((size_t)lane_id * db.nstreams_alloc + s) * 16 + j) * (PX_MAX + 64);
    uint32_t *out = db.px_ring + (((size_t)s * db.px_slots + job.slot) * 2 + ch) * PX_WORDS;
    viterbi_k7_decode(coded, len, dec, out);
    __threadfence_block();
    __syncthreads();
    for (int w = threadIdx.x; w < len / 32; w += 64) out[w] ^= tb.scr_p1[w];
    if (threadIdx.x == 0) { job.pad = db.l2_px_ring ? 1 : 0; job.rec = -1; }     // pad: k_l2_index_px_window owes this frame its index
}

void launch_px_decode(const DevTables &tb, const DevBuffers &db, int nstreams, const int *stream_ids, int parity, int lane_id, hipStream_t st)
{
    hipLaunchKernelGGL(k_px_decode, dim3(16, nstreams), dim3(64), 0, st, tb, db, stream_ids, parity, lane_id);
    if (db.l2_px_ring) launch_l2_index_px_window(db, nstreams, stream_ids, parity, st);
}

}  // namespace nrsc5
