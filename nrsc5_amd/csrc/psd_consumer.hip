// Host side of the PSD transport (nrsc5hip_psd_*): replays block records like nrsc5hip_hdc_feed, but the frames stay in HBM -- one L2
// index launch into device buffers (l2_launch), one k_psd launch over them (k_psd.hip), and only the finished AAS packets come back.
//   per call, device -> host: 4 bytes of PCI per frame (which frames carry fixed-data sub-channels), the arena header (16 bytes), the used
//   part of the arena (12 bytes + the packet, padded to 4, per packet); index and PDU bytes of a frame only where its PCI announces fixed data
// The fixed-data cut needs process_fixed_data's CCC state machine, which is host code (hdc_consumer.hip): the consumer keeps a private
// nrsc5hip_hdc for it and hands k_psd the number of PDUs in front of the cut.
#include <algorithm>
#include <memory>
#include "engine_internal.h"
#include "arena_consumer.h"
#include "record_jobs.h"

struct nrsc5hip_psd {
    int device = 0, nstreams = 0;
    DevFixed<uint8_t> bufs; DevFixed<int> idx; DevFixed<unsigned long long> stats;          // device: PsdArgs
    nrsc5hip_hdc *ccc = nullptr;                                // process_fixed_data's state per stream and logical channel, nothing else of it is used
    DevGrow words, ljobs, frames, bytes;
    ArenaHost ar;
};

static void psd_free(nrsc5hip_psd *p)
{
    if (!p) return;
    nrsc5::DeviceGuard g(p->device);
    nrsc5hip_hdc_destroy(p->ccc);
    delete p;
}

extern "C" int nrsc5hip_psd_create(nrsc5hip_engine *e, int nstreams, nrsc5hip_psd **out)
{
    ON_ENGINE_DEVICE(e);
    if (!out || nstreams < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    nrsc5hip_psd *p = new (std::nothrow) nrsc5hip_psd();
    if (!p) return NRSC5HIP_ENOMEM;
    p->device = e->cfg.device; p->nstreams = nstreams;
    const size_t S = (size_t)nstreams;
    if (nrsc5hip_hdc_create(nstreams, &p->ccc) != 0) { psd_free(p); return NRSC5HIP_ENOMEM; }
    HIPCHK_OR(hipMalloc((void **)&p->bufs.p, S * PSD_PROGRAMS * PSD_MAX_AAS), psd_free(p));
    HIPCHK_OR(hipMalloc((void **)&p->idx.p, S * PSD_PROGRAMS * sizeof(int)), psd_free(p));
    HIPCHK_OR(hipMalloc((void **)&p->stats.p, S * PSD_STATS * sizeof(unsigned long long)), psd_free(p));
    HIPCHK_OR(hipMemset(p->idx.p, 0xff, S * PSD_PROGRAMS * sizeof(int)), psd_free(p));        // -1: closed (frame_reset)
    HIPCHK_OR(hipMemset(p->stats.p, 0, S * PSD_STATS * sizeof(unsigned long long)), psd_free(p));
    HIPCHK_OR(hipDeviceSynchronize(), psd_free(p));
    *out = p;
    return NRSC5HIP_OK;
}

extern "C" void nrsc5hip_psd_destroy(nrsc5hip_psd *p) { psd_free(p); }

extern "C" int nrsc5hip_psd_reset(nrsc5hip_psd *p, int stream)
{
    if (!p || stream < 0 || stream >= p->nstreams) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream");
    nrsc5::DeviceGuard g(p->device);
    HIPCHK(hipMemset(p->idx.p + (size_t)stream * PSD_PROGRAMS, 0xff, PSD_PROGRAMS * sizeof(int)));
    HIPCHK(hipDeviceSynchronize());
    return NRSC5HIP_OK;
}

extern "C" int nrsc5hip_psd_stats(nrsc5hip_psd *p, int stream, long long stats[10])
{
    if (!p || !stats || stream < 0 || stream >= p->nstreams) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream");
    nrsc5::DeviceGuard g(p->device);
    return read_stats<PSD_STATS>(p->stats.p + (size_t)stream * PSD_STATS, p->ar.d2h, stats);
}

// The device work of one call and the delivery: dj[k] = frame k's words in device memory, lcs[k] its logical channel; streams / jobs: what k_psd walks
// (PsdJob::keep is filled in here).  Nothing of the consumer's device state has been touched when this returns an error in front of the k_psd launch.
static int psd_run(nrsc5hip_psd *p, nrsc5hip_engine *e, const std::vector<L2Job> &dj, const std::vector<int> &lcs, std::vector<ArenaStream> &streams,
                   std::vector<PsdJob> &jobs, nrsc5hip_aas_cb cb, void *opaque, const PsdChain *chain)
{
    const size_t n = dj.size(), ns = streams.size();
    if (ns == 0 || jobs.empty()) return 0;
    long long stride = 16;
    if (n) {
        int max_bits = 0;
        for (const L2Job &j : dj) if (j.nbits > max_bits) max_bits = j.nbits;
        stride = ((long long)max_bits / 8 + 15) & ~15LL;        // >= the PDU bytes of the longest frame of this call
        int rc;
        if ((rc = p->ljobs.need(n * sizeof(L2Job))) || (rc = p->frames.need(n * sizeof(nrsc5hip_l2_frame))) || (rc = p->bytes.need(n * (size_t)stride))) return rc;
        if ((rc = l2_launch(e, dj, (L2Job *)p->ljobs.p, (nrsc5hip_l2_frame *)p->frames.p, (uint8_t *)p->bytes.p, stride))) return rc;
        // which frames announce fixed-data sub-channels: the PCI word of every index, nothing else of it
        std::vector<uint32_t> pci(n);
        HIPCHK(hipMemcpy2DAsync(pci.data(), sizeof(uint32_t), (const char *)p->frames.p + offsetof(nrsc5hip_l2_frame, pci), sizeof(nrsc5hip_l2_frame),
                                sizeof(uint32_t), n, hipMemcpyDeviceToHost, e->main));
        HIPCHK(hipStreamSynchronize(e->main));
        p->ar.d2h += (long long)(n * sizeof(uint32_t));
        std::unique_ptr<nrsc5hip_l2_frame> ix;
        std::vector<uint8_t> by;
        for (const ArenaStream &s : streams)
            for (int j = s.first; j < s.first + s.count; j++) {
                PsdJob &job = jobs[j];
                if (job.reset) (void)nrsc5hip_hdc_frame_reset(p->ccc, s.target);          // sync.c:405-409
                if (job.frame < 0) continue;
                const uint32_t w = pci[job.frame];
                const bool fixed_only = (w & 0xFFFFFCu) == (0x3634CEu & 0xFFFFFCu);
                if (!fixed_only && !NRSC5HIP_L2_PCI_HAS_FIXED(w)) continue;
                if (!ix) { ix.reset(new nrsc5hip_l2_frame); by.resize((size_t)stride); }
                HIPCHK(hipMemcpy(ix.get(), (const nrsc5hip_l2_frame *)p->frames.p + job.frame, sizeof(nrsc5hip_l2_frame), hipMemcpyDeviceToHost));
                const unsigned nb = ix->nbytes <= (unsigned)stride ? ix->nbytes : (unsigned)stride;
                HIPCHK(hipMemcpy(by.data(), (const uint8_t *)p->bytes.p + (size_t)job.frame * (size_t)stride, nb, hipMemcpyDeviceToHost));
                p->ar.d2h += (long long)sizeof(nrsc5hip_l2_frame) + nb;
                // PCI_FIXED frames carry no audio, but frame_process runs process_fixed_data on them first (nrsc5hip_hdc_push_frame does the same)
                const unsigned audio_end = nrsc5hip_hdc_fixed_audio_end(p->ccc, s.target, lcs[job.frame], by.data(), nb);
                if (fixed_only) continue;
                const int kept = nrsc5hip_l2_apply_audio_end(ix.get(), audio_end);
                if (kept < 0) FAIL(NRSC5HIP_EINVAL, "a header expansion runs into the fixed-data region: walk that frame on the host");
                job.keep = kept;
            }
    }
    // the plan (streams, jobs) and the arena: sized from what the host knows -- at most 16 PDUs x 255 bytes of new PSD per frame and the 8 x 8212 bytes a
    // stream may carry; a packet of `len` data bytes took len + 8 raw bytes at least (flag, protocol, port, seq, FCS) and takes 12 + len + 3 at most
    size_t raw = 0;
    for (const ArenaStream &s : streams) raw += (size_t)PSD_PROGRAMS * PSD_MAX_AAS + (size_t)s.count * NRSC5HIP_L2_MAX_PDUS * 255;
    const size_t arena_cap = 2 * raw;
    if (arena_cap > 0xfffffff0u) FAIL(NRSC5HIP_EINVAL, "too many frames for one call");
    auto launch = [&](const ArenaDev &d) {
        PsdArgs a;
        a.streams = d.streams; a.jobs = (const PsdJob *)d.jobs; a.njobs = (int)jobs.size();
        a.frames = (const nrsc5hip_l2_frame *)p->frames.p; a.bytes = (const uint8_t *)p->bytes.p; a.stride = stride; a.nframes = (int)n;
        a.bufs = p->bufs.p; a.idx = p->idx.p; a.stats = p->stats.p;
        a.hdr = d.hdr; a.arena = d.arena; a.arena_cap = d.cap;
        launch_psd(a, (int)ns, e->main);
    };
    if (chain) {                                                // the packets stay where k_psd leaves them
        ArenaDev d;
        const int rc = arena_begin(p->ar, e->main, streams, jobs.data(), jobs.size() * sizeof(PsdJob), arena_cap, launch, &d);
        return rc ? rc : (*chain)(d, streams);
    }
    return arena_round<PsdPacket>(p->ar, e->main, "packet", "k_psd", streams, jobs.data(), jobs.size() * sizeof(PsdJob), arena_cap, launch,
                                  [](const PsdPacket &) { return true; }, [&](const ArenaStream &s, const PsdPacket &pk, const uint8_t *data) {
                                      if (cb) cb(opaque, s.target, pk.program, pk.port, pk.seq, data, pk.len);
                                  });
}

// A loss of sync changes nothing here either (see nrsc5hip_hdc_feed): psd_buf / psd_idx are cleared by frame_reset on the NEXT transition to fine sync.
int psd_feed_chain(nrsc5hip_psd *p, nrsc5hip_engine *e, int nstreams, const int *stream_ids, const int *targets, const nrsc5hip_record *const *records,
                   const int *counts, int mode, nrsc5hip_aas_cb cb, void *opaque, const PsdChain *chain)
{
    ON_ENGINE_DEVICE(e);
    if (!p || nstreams < 0 || (mode != NRSC5HIP_MODE_FM && mode != NRSC5HIP_MODE_AM)) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream count / mode");
    if (p->device != e->cfg.device) FAIL(NRSC5HIP_EINVAL, "the consumer was created on another engine's device");
    if (nstreams == 0) return 0;
    if (!stream_ids || !records || !counts) FAIL(NRSC5HIP_EINVAL, "null argument");
    size_t nframes = 0;
    for (int i = 0; i < nstreams; i++) {
        const int t = targets ? targets[i] : stream_ids[i];
        if (stream_ids[i] < 0 || stream_ids[i] >= e->cfg.max_streams || t < 0 || t >= p->nstreams) FAIL(NRSC5HIP_EINVAL, "stream id out of range");
        if (counts[i] < 0 || (counts[i] > 0 && !records[i])) FAIL(NRSC5HIP_EINVAL, "records of stream %d missing", stream_ids[i]);
        for (int k = 0; k < counts[i]; k++) nframes += (size_t)record_jobs(records[i][k], stream_ids[i], mode, nullptr, nullptr);
    }
    int rc = check_targets(p->nstreams, nstreams, targets ? targets : stream_ids); if (rc) return rc;
    if (nframes > (size_t)INT32_MAX / 2) FAIL(NRSC5HIP_EINVAL, "too many frames for one call");
    std::vector<nrsc5hip_l2_job> l2(nframes);
    std::vector<int> lcs(nframes);
    std::vector<ArenaStream> streams;
    std::vector<PsdJob> jobs;
    size_t next = 0;
    for (int i = 0; i < nstreams; i++) {
        const int t = targets ? targets[i] : stream_ids[i];
        const int first = (int)jobs.size();
        for (int k = 0; k < counts[i]; k++) {
            const nrsc5hip_record &r = records[i][k];
            int reset = (r.flags & NRSC5HIP_REC_TO_FINE) ? 1 : 0;                           // before this record's frames
            const int nf = record_jobs(r, stream_ids[i], mode, &l2[next], &lcs[next]);
            for (int f = 0; f < nf; f++, next++) { jobs.push_back(PsdJob{(int)next, NRSC5HIP_L2_MAX_PDUS, reset, 0}); reset = 0; }
            if (reset) jobs.push_back(PsdJob{-1, 0, 1, 0});
        }
        if ((int)jobs.size() > first) streams.push_back(ArenaStream{t, first, (int)jobs.size() - first, (int)streams.size()});
    }
    std::vector<L2Job> dj;
    if (nframes) {
        // every slot / channel / length the records name, before the consumer is touched
        if ((rc = l2_resolve(e, (int)nframes, l2.data(), dj))) return rc;
        HIPCHK(hipDeviceSynchronize());                         // the frames may still be in flight on a decode stream
    }
    return psd_run(p, e, dj, lcs, streams, jobs, cb, opaque, chain);
}

extern "C" int nrsc5hip_psd_feed(nrsc5hip_psd *p, nrsc5hip_engine *e, int nstreams, const int *stream_ids, const int *targets,
                                 const nrsc5hip_record *const *records, const int *counts, int mode, nrsc5hip_aas_cb cb, void *opaque)
{
    return psd_feed_chain(p, e, nstreams, stream_ids, targets, records, counts, mode, cb, opaque, nullptr);
}

int psd_stage_chain(nrsc5hip_psd *p, nrsc5hip_engine *e, int nstreams, const int *targets, const uint8_t *const *bits, const int *nbits, const int *nframes,
                    const int *lcs, const int *reset_at, nrsc5hip_aas_cb cb, void *opaque, const PsdChain *chain)
{
    ON_ENGINE_DEVICE(e);
    if (!p || nstreams < 1 || !targets || !bits || !nbits || !nframes || !lcs) FAIL(NRSC5HIP_EINVAL, "bad argument");
    if (p->device != e->cfg.device) FAIL(NRSC5HIP_EINVAL, "the consumer was created on another engine's device");
    size_t total_words = 0, total_frames = 0;
    for (int i = 0; i < nstreams; i++) {
        if (targets[i] < 0 || targets[i] >= p->nstreams || !bits[i] || nbits[i] < 1 || nbits[i] > P1_LEN || nframes[i] < 1 || lcs[i] < 0 || lcs[i] > 2)
            FAIL(NRSC5HIP_EINVAL, "stream %d of the call: bad target / frames / length / channel", i);
        if (reset_at && reset_at[i] > nframes[i]) FAIL(NRSC5HIP_EINVAL, "stream %d of the call: reset behind the end", i);
        total_words += (size_t)((nbits[i] + 31) / 32) * nframes[i];
        total_frames += (size_t)nframes[i];
    }
    int rc = check_targets(p->nstreams, nstreams, targets); if (rc) return rc;
    if (total_frames > (size_t)INT32_MAX / 2) FAIL(NRSC5HIP_EINVAL, "too many frames for one call");
    std::vector<uint32_t> w(total_words, 0u);
    if ((rc = p->words.need(w.size() * sizeof(uint32_t)))) return rc;
    std::vector<L2Job> dj;
    std::vector<int> lc;
    std::vector<PsdJob> jobs;
    std::vector<ArenaStream> streams;
    size_t at = 0;
    for (int i = 0; i < nstreams; i++) {
        const int words = (nbits[i] + 31) / 32, first = (int)jobs.size(), rst = reset_at ? reset_at[i] : -1;
        for (int f = 0; f < nframes[i]; f++, at += words) {
            for (int k = 0; k < nbits[i]; k++) w[at + (k >> 5)] |= (uint32_t)(bits[i][(size_t)f * nbits[i] + k] & 1u) << (k & 31);
            jobs.push_back(PsdJob{(int)dj.size(), NRSC5HIP_L2_MAX_PDUS, f == rst ? 1 : 0, 0});
            dj.push_back(L2Job{(const uint32_t *)p->words.p + at, nbits[i], 0});
            lc.push_back(lcs[i]);
        }
        if (rst == nframes[i]) jobs.push_back(PsdJob{-1, 0, 1, 0});          // as a REC_TO_FINE record that announces no frame
        streams.push_back(ArenaStream{targets[i], first, (int)jobs.size() - first, i});
    }
    HIPCHK(hipMemcpy(p->words.p, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return psd_run(p, e, dj, lc, streams, jobs, cb, opaque, chain);
}

extern "C" int nrsc5hip_stage_psd_streams(nrsc5hip_psd *p, nrsc5hip_engine *e, int nstreams, const int *targets, const uint8_t *const *bits, const int *nbits,
                                          const int *nframes, const int *lcs, const int *reset_at, nrsc5hip_aas_cb cb, void *opaque)
{
    return psd_stage_chain(p, e, nstreams, targets, bits, nbits, nframes, lcs, reset_at, cb, opaque, nullptr);
}

extern "C" int nrsc5hip_stage_psd(nrsc5hip_psd *p, nrsc5hip_engine *e, int stream, const uint8_t *bits, int nbits, int nframes, int lc,
                                  nrsc5hip_aas_cb cb, void *opaque)
{
    return nrsc5hip_stage_psd_streams(p, e, 1, &stream, &bits, &nbits, &nframes, &lc, nullptr, cb, opaque);
}
