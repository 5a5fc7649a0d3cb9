// Host side of the data services on the device (nrsc5hip_aas_*): chains one k_aas launch (k_aas.hip) behind the PSD consumer's k_psd launch -- the packet
// arena stays in HBM -- and hands the events of its own arena to the caller.
//   per call, host -> device: the plan (16 bytes per listed stream), beside what the PSD consumer uploads
//   per call, device -> host: the arena header (16 bytes) and the used part of the event arena (48 bytes + the data, padded to 4, per event)
#include <algorithm>
#include "engine_internal.h"
#include "arena_consumer.h"

struct nrsc5hip_aas {
    int device = 0, nstreams = 0, lot_files = 0, flags = 0;
    DevFixed<AasStream> state; DevFixed<AasFile> files; DevFixed<uint8_t> data; DevFixed<unsigned long long> stats;     // device: AasArgs
    DevGrow packets;                                                // stage hook: the uploaded packet arena
    ArenaHost ar;
    long long arena_limit = 0;                                      // test hook: 0 = the host-known bound
};

static void aas_free(nrsc5hip_aas *a)
{
    if (!a) return;
    nrsc5::DeviceGuard g(a->device);
    delete a;
}

static int aas_clear(nrsc5hip_aas *a, int stream)
{
    AasStream st;
    memset(&st, 0, sizeof(st));
    st.lot_lru_counter = 1;                                         // aas_reset, output.c:198
    HIPCHK(hipMemcpy(a->state.p + stream, &st, sizeof(st), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(a->files.p + (size_t)stream * a->lot_files, 0, (size_t)a->lot_files * sizeof(AasFile)));       // timestamp 0: free
    return NRSC5HIP_OK;
}

extern "C" int nrsc5hip_aas_create(nrsc5hip_engine *e, int nstreams, int lot_files, int flags, nrsc5hip_aas **out)
{
    ON_ENGINE_DEVICE(e);
    if (!out || nstreams < 1 || lot_files < 1 || lot_files > AAS_MAX_FILES || (flags & ~NRSC5HIP_AAS_FRAGMENTS)) FAIL(NRSC5HIP_EINVAL, "bad argument");
    nrsc5hip_aas *a = new (std::nothrow) nrsc5hip_aas();
    if (!a) return NRSC5HIP_ENOMEM;
    a->device = e->cfg.device; a->nstreams = nstreams; a->lot_files = lot_files; a->flags = flags;
    const size_t S = (size_t)nstreams, F = S * (size_t)lot_files;
    HIPCHK_OR(hipMalloc((void **)&a->state.p, S * sizeof(AasStream)), aas_free(a));
    HIPCHK_OR(hipMalloc((void **)&a->files.p, F * sizeof(AasFile)), aas_free(a));
    HIPCHK_OR(hipMalloc((void **)&a->data.p, F * AAS_FILE_BYTES), aas_free(a));
    HIPCHK_OR(hipMalloc((void **)&a->stats.p, S * AAS_STATS * sizeof(unsigned long long)), aas_free(a));
    HIPCHK_OR(hipMemset(a->stats.p, 0, S * AAS_STATS * sizeof(unsigned long long)), aas_free(a));
    for (int s = 0; s < nstreams; s++)
        if (aas_clear(a, s) != NRSC5HIP_OK) { aas_free(a); return NRSC5HIP_EHIP; }
    HIPCHK_OR(hipDeviceSynchronize(), aas_free(a));
    *out = a;
    return NRSC5HIP_OK;
}

extern "C" void nrsc5hip_aas_destroy(nrsc5hip_aas *a) { aas_free(a); }

extern "C" int nrsc5hip_aas_reset(nrsc5hip_aas *a, int stream)
{
    if (!a || stream < 0 || stream >= a->nstreams) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream");
    nrsc5::DeviceGuard g(a->device);
    int rc = aas_clear(a, stream); if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    return NRSC5HIP_OK;
}

extern "C" int nrsc5hip_aas_debug_arena(nrsc5hip_aas *a, long long bytes)
{
    if (!a || bytes < 0) FAIL(NRSC5HIP_EINVAL, "bad consumer / size");
    a->arena_limit = bytes;
    return NRSC5HIP_OK;
}

extern "C" int nrsc5hip_aas_stats(nrsc5hip_aas *a, int stream, long long stats[NRSC5HIP_AAS_NSTATS])
{
    if (!a || !stats || stream < 0 || stream >= a->nstreams) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream");
    nrsc5::DeviceGuard g(a->device);
    return read_stats<AAS_STATS>(a->stats.p + (size_t)stream * AAS_STATS, a->ar.d2h, stats);
}

extern "C" int nrsc5hip_aas_sig(nrsc5hip_aas *a, int stream, uint8_t *out, unsigned *len, int *nservices)
{
    if (!a || !out || !len || !nservices || stream < 0 || stream >= a->nstreams) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream");
    nrsc5::DeviceGuard g(a->device);
    std::vector<AasStream> st(1);
    HIPCHK(hipMemcpy(st.data(), a->state.p + stream, sizeof(AasStream), hipMemcpyDeviceToHost));
    unsigned ns = 0;
    *len = aas_sig_flatten(st[0].services, out, &ns);
    *nservices = (int)ns;
    return NRSC5HIP_OK;
}

// One k_aas launch on `st` over the packet arena `in` (device memory: header, records, capacity) whose records carry the positions of `streams`, and the delivery
static int aas_run(nrsc5hip_aas *a, hipStream_t st, const ArenaDev &in, const std::vector<ArenaStream> &streams, nrsc5hip_aas_event_cb cb, void *opaque)
{
    if (streams.empty()) return 0;
    // the event arena, from what the host knows (include/nrsc5hip.h, nrsc5hip_aas_feed)
    const size_t bound = 4 * (size_t)in.cap + streams.size() * (8192 + (size_t)a->lot_files * (AAS_FILE_BYTES + 512));
    if (bound > 0xfffffff0u) FAIL(NRSC5HIP_EINVAL, "too many frames for one call");
    const size_t arena_cap = a->arena_limit ? std::min<size_t>(bound, (size_t)a->arena_limit) : bound;
    auto launch = [&](const ArenaDev &d) {
        AasArgs k;
        k.streams = d.streams; k.nstreams = a->nstreams; k.lot_files = a->lot_files; k.flags = a->flags;
        k.in_hdr = in.hdr; k.in_arena = in.arena; k.in_cap = in.cap;
        k.state = a->state.p; k.files = a->files.p; k.data = a->data.p; k.stats = a->stats.p;
        k.hdr = d.hdr; k.arena = d.arena; k.arena_cap = d.cap;
        launch_aas(k, (int)streams.size(), st);
    };
    return arena_round<AasEvent>(a->ar, st, "event", "k_aas", streams, nullptr, 0, arena_cap, launch,
                                 [](const AasEvent &ev) { return ev.kind >= NRSC5HIP_AAS_PSD && ev.kind <= NRSC5HIP_AAS_PACKET; },
                                 [&](const ArenaStream &s, const AasEvent &ev, const uint8_t *data) {
                                     if (cb) cb(opaque, s.target, ev.kind, ev.port, ev.seq, ev.v, data, ev.len);
                                 });
}

static int aas_check_chain(nrsc5hip_aas *a, nrsc5hip_psd *psd, nrsc5hip_engine *e, int nstreams, const int *targets)
{
    if (!a || !psd || !e) FAIL(NRSC5HIP_EINVAL, "null consumer / engine");
    if (a->device != e->cfg.device) FAIL(NRSC5HIP_EINVAL, "the consumer was created on another engine's device");
    for (int i = 0; targets && i < nstreams; i++)
        if (targets[i] < 0 || targets[i] >= a->nstreams) FAIL(NRSC5HIP_EINVAL, "consumer stream %d out of range", targets[i]);
    return 0;
}

extern "C" int nrsc5hip_aas_feed(nrsc5hip_aas *a, nrsc5hip_psd *psd, nrsc5hip_engine *e, int nstreams, const int *stream_ids, const int *targets,
                                 const nrsc5hip_record *const *records, const int *counts, int mode, nrsc5hip_aas_event_cb cb, void *opaque)
{
    if (nstreams > 0 && !stream_ids) FAIL(NRSC5HIP_EINVAL, "null argument");
    int rc = aas_check_chain(a, psd, e, nstreams, targets ? targets : stream_ids); if (rc) return rc;
    const PsdChain chain = [&](const ArenaDev &in, const std::vector<ArenaStream> &streams) { return aas_run(a, e->main, in, streams, cb, opaque); };
    return psd_feed_chain(psd, e, nstreams, stream_ids, targets, records, counts, mode, nullptr, nullptr, &chain);
}

extern "C" int nrsc5hip_stage_aas_frames(nrsc5hip_aas *a, nrsc5hip_psd *psd, nrsc5hip_engine *e, int nstreams, const int *targets, const uint8_t *const *bits,
                                         const int *nbits, const int *nframes, const int *lcs, const int *reset_at, nrsc5hip_aas_event_cb cb, void *opaque)
{
    if (nstreams > 0 && !targets) FAIL(NRSC5HIP_EINVAL, "null argument");
    int rc = aas_check_chain(a, psd, e, nstreams, targets); if (rc) return rc;
    const PsdChain chain = [&](const ArenaDev &in, const std::vector<ArenaStream> &streams) { return aas_run(a, e->main, in, streams, cb, opaque); };
    return psd_stage_chain(psd, e, nstreams, targets, bits, nbits, nframes, lcs, reset_at, nullptr, nullptr, &chain);
}

extern "C" int nrsc5hip_stage_aas(nrsc5hip_aas *a, int nstreams, const int *targets, const uint8_t *const *packets, const int *nbytes,
                                  nrsc5hip_aas_event_cb cb, void *opaque)
{
    if (!a || nstreams < 1 || !packets || !nbytes) FAIL(NRSC5HIP_EINVAL, "bad argument");
    nrsc5::DeviceGuard g(a->device);
    int rc = check_targets(a->nstreams, nstreams, targets); if (rc) return rc;
    // per stream the records, then one arena: packet k of every stream, then packet k + 1
    std::vector<std::vector<std::vector<uint8_t>>> recs((size_t)nstreams);
    std::vector<ArenaStream> streams;
    size_t total = 0, most = 0;
    for (int i = 0; i < nstreams; i++) {
        if (nbytes[i] < 0 || (nbytes[i] > 0 && !packets[i])) FAIL(NRSC5HIP_EINVAL, "stream %d of the call: packets missing", i);
        for (size_t at = 0; at < (size_t)nbytes[i];) {
            const uint8_t *q = packets[i] + at;
            if (at + 8 > (size_t)nbytes[i]) FAIL(NRSC5HIP_EINVAL, "stream %d of the call: a packet header runs past the end", i);
            PsdPacket p;
            p.pos = (uint32_t)i; p.port = (uint16_t)(q[0] | (q[1] << 8)); p.seq = (uint16_t)(q[2] | (q[3] << 8)); p.len = (uint16_t)(q[4] | (q[5] << 8));
            p.program = q[6]; p.pad = 0;
            if (at + 8 + p.len > (size_t)nbytes[i]) FAIL(NRSC5HIP_EINVAL, "stream %d of the call: a packet runs past the end", i);
            std::vector<uint8_t> r(sizeof(PsdPacket) + (((size_t)p.len + 3) & ~(size_t)3), 0);
            memcpy(r.data(), &p, sizeof(p));
            memcpy(r.data() + sizeof(p), q + 8, p.len);
            total += r.size();
            recs[i].push_back(std::move(r));
            at += 8 + (size_t)p.len;
        }
        most = std::max(most, recs[i].size());
        streams.push_back(ArenaStream{targets ? targets[i] : i, 0, 0, i});
    }
    if (total > 0x3ffffff0u) FAIL(NRSC5HIP_EINVAL, "too many packets for one call");
    std::vector<uint8_t> arena(sizeof(ArenaHdr) + total);
    ArenaHdr hdr{(unsigned)total, 0, 0, 0};
    size_t at = sizeof(ArenaHdr);
    for (size_t k = 0; k < most; k++)
        for (int i = 0; i < nstreams; i++)
            if (k < recs[i].size()) { memcpy(arena.data() + at, recs[i][k].data(), recs[i][k].size()); at += recs[i][k].size(); hdr.count++; }
    memcpy(arena.data(), &hdr, sizeof(hdr));
    if ((rc = a->packets.need(arena.size()))) return rc;
    HIPCHK(hipMemcpy(a->packets.p, arena.data(), arena.size(), hipMemcpyHostToDevice));
    const ArenaDev in{nullptr, nullptr, (ArenaHdr *)a->packets.p, (uint8_t *)a->packets.p + sizeof(ArenaHdr), (unsigned)total};
    return aas_run(a, nullptr, in, streams, cb, opaque);
}
