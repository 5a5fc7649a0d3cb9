// Host plumbing of the arena consumers (psd_consumer.hip, sis_consumer.hip; the device side of the contract: kernels.h, ArenaStream / ArenaHdr):
// device buffers that free themselves, the target check, one plan / arena round and the stats read-back.
#pragma once
#include <string.h>
#include <functional>
#include <vector>
#include "kernels.h"
#include "host_util.h"

namespace nrsc5 {

struct DevGrow {                                                // a device buffer that only ever grows; kept between calls
    void *p = nullptr; size_t cap = 0;
    ~DevGrow() { if (p) (void)hipFree(p); }
    int need(size_t n)
    {
        if (n <= cap) return 0;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        n += n / 4;
        hipError_t err = hipMalloc(&p, n);
        if (err != hipSuccess) { p = nullptr; FAIL(NRSC5HIP_ENOMEM, "hipMalloc(%zu bytes) failed: %s", n, hipGetErrorString(err)); }
        cap = n;
        return 0;
    }
};

template <typename T> struct DevFixed { T *p = nullptr; ~DevFixed() { if (p) (void)hipFree(p); } };   // a device array of fixed size, freed with its owner
struct ArenaHost { DevGrow plan, arena; long long d2h = 0; };   // what a consumer keeps for its rounds; d2h: bytes its feeds copied device -> host
struct ArenaDev { const ArenaStream *streams; const void *jobs; ArenaHdr *hdr; uint8_t *arena; unsigned cap; };   // a round's device pointers, for the launch

// the consumer streams a call lists (targets[i], or i without a list): each inside the consumer and listed once
inline int check_targets(int consumer_streams, int n, const int *targets)
{
    std::vector<char> seen((size_t)consumer_streams, 0);
    for (int i = 0; i < n; i++) {
        const int t = targets ? targets[i] : i;
        if (t < 0 || t >= consumer_streams) FAIL(NRSC5HIP_EINVAL, "consumer stream %d out of range", t);
        if (seen[t]) FAIL(NRSC5HIP_EINVAL, "consumer stream %d listed twice", t);          // two workgroups would walk one state
        seen[t] = 1;
    }
    return 0;
}

// nrsc5hip_*_stats: the N device counters of a stream, then d2h
template <int N> int read_stats(const unsigned long long *dev, long long d2h, long long *out)
{
    unsigned long long v[N];
    HIPCHK(hipMemcpy(v, dev, sizeof(v), hipMemcpyDeviceToHost));
    for (int k = 0; k < N; k++) out[k] = (long long)v[k];
    out[N] = d2h;
    return NRSC5HIP_OK;
}

// The records in the used part of an arena (no HIP in here): per[pos] = the offsets of that stream's records, in arena order.  Rec: the record header, with
// `pos` and `len`; valid(rec): the consumer's own test, made once pos is known to be inside the list.  -> false and *bad = the offset of a record the kernel
// cannot have written
template <typename Rec, typename Valid>
bool arena_walk(const uint8_t *got, size_t used, size_t ns, Valid valid, std::vector<std::vector<size_t>> &per, size_t *bad)
{
    per.assign(ns, std::vector<size_t>());
    for (size_t at = 0; at + sizeof(Rec) <= used;) {
        Rec r;
        memcpy(&r, got + at, sizeof(r));
        const size_t rec = sizeof(Rec) + (((size_t)r.len + 3) & ~(size_t)3);
        if (r.pos >= ns || at + rec > used || !valid(r)) { *bad = at; return false; }
        per[r.pos].push_back(at);
        at += rec;
    }
    return true;
}

// The first half of a round on `st`: grows plan and arena (nothing has been touched when that fails), uploads the plan (streams, then job_bytes of jobs) in
// one copy, clears the header and runs launch(ArenaDev).  *out: the round's device pointers, for arena_collect or for a consumer chained behind it
template <typename Launch>
int arena_begin(ArenaHost &h, hipStream_t st, const std::vector<ArenaStream> &streams, const void *jobs, size_t job_bytes, size_t arena_cap, Launch launch, ArenaDev *out)
{
    const size_t ns = streams.size(), plan_streams = ns * sizeof(ArenaStream), plan_bytes = plan_streams + job_bytes;
    int rc;
    if ((rc = h.plan.need(plan_bytes)) || (rc = h.arena.need(sizeof(ArenaHdr) + arena_cap))) return rc;
    std::vector<uint8_t> plan(plan_bytes);
    memcpy(plan.data(), streams.data(), plan_streams);
    if (job_bytes) memcpy(plan.data() + plan_streams, jobs, job_bytes);
    HIPCHK(hipMemcpy(h.plan.p, plan.data(), plan_bytes, hipMemcpyHostToDevice));
    HIPCHK(st ? hipMemsetAsync(h.arena.p, 0, sizeof(ArenaHdr), st) : hipMemset(h.arena.p, 0, sizeof(ArenaHdr)));
    const ArenaDev d{(const ArenaStream *)h.plan.p, (const uint8_t *)h.plan.p + plan_streams, (ArenaHdr *)h.arena.p, (uint8_t *)h.arena.p + sizeof(ArenaHdr), (unsigned)arena_cap};
    launch(d);
    HIPCHK(hipGetLastError());
    *out = d;
    return 0;
}

// The second half: reads the header and then the used part, and hands every record to deliver(stream, rec, its bytes): all of the first listed stream's
// records first -- the arena holds each stream's records in order, the streams interleaved.  what / kernel: for the texts.  -> records delivered, or < 0
template <typename Rec, typename Valid, typename Deliver>
int arena_collect(ArenaHost &h, hipStream_t st, const char *what, const char *kernel, const std::vector<ArenaStream> &streams, const ArenaDev &d, Valid valid, Deliver deliver)
{
    const size_t ns = streams.size(), arena_cap = d.cap;
    ArenaHdr hdr;
    if (st) {
        HIPCHK(hipMemcpyAsync(&hdr, h.arena.p, sizeof(hdr), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    } else HIPCHK(hipMemcpy(&hdr, h.arena.p, sizeof(hdr), hipMemcpyDeviceToHost));      // null stream: the blocking forms (measured ~20 us per call shorter on the MI355X)
    h.d2h += (long long)sizeof(hdr);
    if (hdr.overflow || hdr.used > arena_cap) FAIL(NRSC5HIP_EOVERFLOW, "%s arena of %zu bytes too small (%u needed): %ss of this call are lost", what, arena_cap, hdr.used, what);
    if (hdr.used == 0) return 0;
    std::vector<uint8_t> got(hdr.used);
    HIPCHK(hipMemcpy(got.data(), d.arena, hdr.used, hipMemcpyDeviceToHost));
    h.d2h += hdr.used;
    std::vector<std::vector<size_t>> per;
    size_t bad = 0;
    if (!arena_walk<Rec>(got.data(), got.size(), ns, valid, per, &bad)) FAIL(NRSC5HIP_EHIP, "%s arena is not what %s writes (offset %zu)", what, kernel, bad);
    int delivered = 0;
    for (size_t i = 0; i < ns; i++)
        for (size_t at : per[i]) {
            Rec r;
            memcpy(&r, got.data() + at, sizeof(r));
            deliver(streams[i], r, got.data() + at + sizeof(Rec));
            delivered++;
        }
    return delivered;
}

// One round: arena_begin, then arena_collect
template <typename Rec, typename Launch, typename Valid, typename Deliver>
int arena_round(ArenaHost &h, hipStream_t st, const char *what, const char *kernel, const std::vector<ArenaStream> &streams, const void *jobs, size_t job_bytes,
                size_t arena_cap, Launch launch, Valid valid, Deliver deliver)
{
    ArenaDev d;
    const int rc = arena_begin(h, st, streams, jobs, job_bytes, arena_cap, launch, &d);
    return rc ? rc : arena_collect<Rec>(h, st, what, kernel, streams, d, valid, deliver);
}

}  // namespace nrsc5

// What a consumer chained behind k_psd does with the round's packet arena, still in device memory (aas_consumer.hip): -> its result.  The PSD consumer's
// own delivery does not happen then
using PsdChain = std::function<int(const nrsc5::ArenaDev &packets, const std::vector<nrsc5::ArenaStream> &streams)>;
// nrsc5hip_psd_feed / nrsc5hip_stage_psd_streams; chain == nullptr: exactly those
int psd_feed_chain(nrsc5hip_psd *p, nrsc5hip_engine *e, int nstreams, const int *stream_ids, const int *targets, const nrsc5hip_record *const *records,
                   const int *counts, int mode, nrsc5hip_aas_cb cb, void *opaque, const PsdChain *chain);
int psd_stage_chain(nrsc5hip_psd *p, nrsc5hip_engine *e, int nstreams, const int *targets, const uint8_t *const *bits, const int *nbits, const int *nframes,
                    const int *lcs, const int *reset_at, nrsc5hip_aas_cb cb, void *opaque, const PsdChain *chain);
