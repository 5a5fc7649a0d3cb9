// The logical frames a block record announces, as L2 index jobs: shared by the consumers that replay records (nrsc5hip_hdc_feed in
// hdc_consumer.hip, nrsc5hip_psd_feed in psd_consumer.hip).  Host code only.
#pragma once
#include "nrsc5hip.h"

namespace nrsc5 {

// in frame_push's order (decode.c:393-437, 507-554); -> how many; job / lc may be null (count only).  lc: the frame's logical channel
// (0 = P1, 1 = P3, 2 = P4), which selects the fixed-data (CCC) state it advances
inline int record_jobs(const nrsc5hip_record &r, int stream, int mode, nrsc5hip_l2_job *job, int *lc)
{
    int n = 0;
    auto add = [&](int slot, int kind, int which, int nbits, int channel) {
        if (job) { job[n] = nrsc5hip_l2_job{stream, slot, kind, which, nbits}; lc[n] = channel; }
        n++;
    };
    if (mode == NRSC5HIP_MODE_AM) {
        if (r.flags & NRSC5HIP_REC_P1) add(r.p1_slot, NRSC5HIP_L2_AM, r.bc_decoded, 3750, 0);
        if (r.flags & NRSC5HIP_REC_P3) add(r.p1_slot, NRSC5HIP_L2_AM, 8, r.psmi == 2 ? 30000 : 24000, 1);
    } else {
        const int px_bits = r.psmi == 2 ? 2304 : 4608;
        if (r.flags & NRSC5HIP_REC_P1) add(r.p1_slot, NRSC5HIP_L2_FM_P1, 0, 146176, 0);
        if (r.flags & NRSC5HIP_REC_P3) add((int)r.sis, NRSC5HIP_L2_FM_PX, 0, px_bits, 1);
        if (r.flags & NRSC5HIP_REC_P4) add((int)r.sis, NRSC5HIP_L2_FM_PX, 1, px_bits, 2);
    }
    return n;
}

}  // namespace nrsc5
