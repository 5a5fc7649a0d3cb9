// Batched FIFO trim (nrsc5hip_batch_trim): give back the slab space in front of everything a stream may still read.
//
// The batch path appends at q15[wr - base] and never moved `base`; the streaming seam's k_compact moves it to `rd`, which the
// replay of the window pipeline (p1_async + l2_feedback, k_replay.hip) cannot live with: k_rollback / k_rollback_am set st.rd
// back to the read position a checkpoint holds, and the samples from there on must still be in the slab.  The floor of a stream
// is therefore
//
//     min( st.rd,
//          ckpt[s][p].rd            for every FM decode window slot p whose frame is still with its deferred decode
//                                   (p1_pending[p] != 0: no verdict yet) or whose verdict "failed" nobody has taken
//                                   (p1_verdict[p] == 2: k_rollback may still be holding it back, NRSC5HIP_TUNE_VERDICT_LAG),
//          am_ckpt[s][p][j].st.rd   for every delivered P1 PDU j (deliver_abs[j] >= 0) of AM job p whose verdict is unknown
//                                   while the job's decodes run (verdict 0, job.valid) or "failed" and not applied (verdict 2) )
//
// A verdict "good" (1), a consumed one (FM 0 with nothing pending, AM 3) and a slot no frame was ever filed in keep nothing:
// k_rollback* never rewinds to them.  Slots of frames whose block was itself rewound over are kept although their verdict
// will be ignored (REC_DISCARDED): more, never less.
//
// The checkpoint terms are DEFENSIVE: with today's scheduler they never lower the floor.  Every nrsc5hip_batch_process -- also one that
// runs out of max_steps -- ends with flush_p1 / am_flush (all deferred decodes done) and a rollback with lag 0 that takes every verdict
// (engine_steps.hip: run_steps, run_steps_am), and a trim is a host call between two of them: p1_pending is 0, no verdict is open and
// floor == st.rd.  They keep the rule right should a scheduler ever return with decodes in flight; no test can reach them through the
// public interface, and the tests would pass the same with floor = st.rd.
//
// Three launches on the chain stream.  k_trim_plan (one work-item per listed stream) computes the floor, files the move
// { off = floor - base, n = wr - floor } and commits st.base = floor; the two move kernels read nothing but the plan, and each
// returns at once for a stream that is the other's.  Source [off, off + n) and destination [0, n) are disjoint when off >= n -- the
// usual case: a trim is called when the slab is full and less than a window is live -- and then every workgroup of the stream's row
// copies its own tiles (k_trim_move).  When they overlap -- a trim while most of the slab is still unread -- one workgroup walks the
// span front to back in passes staged through LDS (k_trim_move_overlap).  The list must not name a stream twice (two rows would move
// the same span concurrently): the entry point rejects that.
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace nrsc5 {

__global__ __launch_bounds__(64) void k_trim_plan(DevBuffers db, const int *ids, int nstreams, TrimPlan *plan)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nstreams) return;
    const int s = stream_of(ids, k);
    StreamState &st = db.state[s];
    TrimPlan pl;
    pl.off = 0; pl.n = 0; pl.base = st.base; pl.wr = st.wr;
    if (st.raw) { plan[k] = pl; return; }                      // the stream reads a capture in place: nothing of it is in the slab
    long long floor = st.rd;
    if (st.mode == MODE_AM) {
        if (db.am_ckpt && db.am_job)
            for (int p = 0; p < NWIN; p++) {
                const AmJob &job = db.am_job[(size_t)s * NWIN + p];
                for (int j = 0; j < 8; j++) {
                    const int v = job.verdict[j];
                    if (job.deliver_abs[j] < 0 || !(v == 2 || (v == 0 && job.valid))) continue;
                    const long long rd = db.am_ckpt[((size_t)s * NWIN + p) * 8 + j].st.rd;
                    if (rd < floor) floor = rd;
                }
            }
    } else if (db.ckpt) {
        for (int p = 0; p < NWIN; p++) {
            if (!st.p1_pending[p] && st.p1_verdict[p] != 2) continue;
            const long long rd = db.ckpt[(size_t)s * NWIN + p].rd;
            if (rd < floor) floor = rd;
        }
    }
    if (floor > pl.wr) floor = pl.wr;
    if (floor > pl.base) {                                     // (a floor at or below base: nothing to give back)
        pl.off = floor - pl.base; pl.n = pl.wr - floor;        // off + n = wr - base <= q15_cap: both ranges lie inside the slab
        pl.base = floor;
        st.base = floor;
    }
    plan[k] = pl;
}

constexpr int TRIM_NT = 256;                                   // work-items per workgroup
constexpr int TRIM_TILE = 4096;                                // disjoint move: c16 samples per tile of a workgroup's grid-stride walk
constexpr int TRIM_STAGE = 12288;                              // overlapping move: samples staged through LDS per pass (48 KiB)

// source [off, off + n) and destination [0, n) are disjoint (off >= n): tiles in any order, by every workgroup of the stream's row
__global__ __launch_bounds__(TRIM_NT) void k_trim_move(DevBuffers db, const int *ids, const TrimPlan *plan)
{
    const int s = stream_of(ids, blockIdx.y);
    const long long off = plan[blockIdx.y].off, n = plan[blockIdx.y].n;
    if (off <= 0 || n <= 0 || off < n) return;                 // block-uniform (off < n: k_trim_move_overlap's)
    uint32_t *buf = (uint32_t *)(db.q15 + (size_t)s * db.q15_cap);   // one c16 = one dword
    const int tid = threadIdx.x;
    for (long long c = (long long)blockIdx.x * TRIM_TILE; c < n; c += (long long)gridDim.x * TRIM_TILE)
        for (int i = tid; i < TRIM_TILE; i += TRIM_NT) {
            const long long q = c + i;
            if (q < n) buf[q] = buf[off + q];
        }
}

// they overlap (0 < off < n): one workgroup per stream walks the span front to back.  A pass reads [off + c, off + c + STAGE) into LDS -- the
// store to LDS needs the loaded value, so behind the barrier every read of the pass has completed -- and then writes [c, c + STAGE); with
// off < STAGE the two ranges of ONE pass overlap, which the staging makes harmless, and a pass's writes end at c + STAGE <= the next pass's
// first read off + c + STAGE: nothing is overwritten before it was read.  The second barrier keeps the next pass's LDS stores behind this
// pass's LDS loads.
__global__ __launch_bounds__(TRIM_NT) void k_trim_move_overlap(DevBuffers db, const int *ids, const TrimPlan *plan)
{
    const int s = stream_of(ids, blockIdx.x);
    const long long off = plan[blockIdx.x].off, n = plan[blockIdx.x].n;
    if (off <= 0 || n <= 0 || off >= n) return;                // block-uniform
    uint32_t *buf = (uint32_t *)(db.q15 + (size_t)s * db.q15_cap);
    const int tid = threadIdx.x;
    __shared__ uint32_t stage[TRIM_STAGE];
    for (long long c = 0; c < n; c += TRIM_STAGE) {
        for (int i = tid; i < TRIM_STAGE; i += TRIM_NT) { const long long q = c + i; if (q < n) stage[i] = buf[off + q]; }
        __syncthreads();
        for (int i = tid; i < TRIM_STAGE; i += TRIM_NT) { const long long q = c + i; if (q < n) buf[q] = stage[i]; }
        __syncthreads();
    }
}

void launch_trim(const DevBuffers &db, int nstreams, const int *stream_ids, TrimPlan *plan, int row_wgs, hipStream_t st)
{
    hipLaunchKernelGGL(k_trim_plan, dim3((nstreams + 63) / 64), dim3(64), 0, st, db, stream_ids, nstreams, plan);
    hipLaunchKernelGGL(k_trim_move, dim3(row_wgs < 1 ? 1 : row_wgs, nstreams), dim3(TRIM_NT), 0, st, db, stream_ids, plan);
    hipLaunchKernelGGL(k_trim_move_overlap, dim3(nstreams), dim3(TRIM_NT), 0, st, db, stream_ids, plan);
}

}  // namespace nrsc5
