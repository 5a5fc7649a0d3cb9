// Host side of SIS on the device (nrsc5hip_sis_*): packs the PIDS words of the block records (16 bytes per record), launches k_sis once over
// all listed streams (k_sis.hip) and hands the events of the arena to the caller.
//   per call, host -> device: the plan (16 bytes per listed stream) and the entries (16 bytes per frame)
//   per call, device -> host: the arena header (16 bytes) and the used part of the arena (48 bytes + the text, padded to 4, per event)
#include <algorithm>
#include "engine_internal.h"
#include "arena_consumer.h"

struct nrsc5hip_sis {
    int device = 0, nstreams = 0;
    DevFixed<SisState> state; DevFixed<unsigned long long> stats;      // device: SisArgs
    ArenaHost ar;
    long long arena_limit = 0;                                      // test hook: 0 = the host-known bound
};

static void sis_free(nrsc5hip_sis *s)
{
    if (!s) return;
    nrsc5::DeviceGuard g(s->device);
    delete s;
}

extern "C" int nrsc5hip_sis_create(nrsc5hip_engine *e, int nstreams, nrsc5hip_sis **out)
{
    ON_ENGINE_DEVICE(e);
    if (!out || nstreams < 1) FAIL(NRSC5HIP_EINVAL, "bad argument");
    nrsc5hip_sis *s = new (std::nothrow) nrsc5hip_sis();
    if (!s) return NRSC5HIP_ENOMEM;
    s->device = e->cfg.device; s->nstreams = nstreams;
    const size_t S = (size_t)nstreams;
    HIPCHK_OR(hipMalloc((void **)&s->state.p, S * sizeof(SisState)), sis_free(s));
    HIPCHK_OR(hipMalloc((void **)&s->stats.p, S * SIS_STATS * sizeof(unsigned long long)), sis_free(s));
    std::vector<SisState> init(S);
    for (SisState &st : init) sis_state_init(st);
    HIPCHK_OR(hipMemcpy(s->state.p, init.data(), S * sizeof(SisState), hipMemcpyHostToDevice), sis_free(s));
    HIPCHK_OR(hipMemset(s->stats.p, 0, S * SIS_STATS * sizeof(unsigned long long)), sis_free(s));
    HIPCHK_OR(hipDeviceSynchronize(), sis_free(s));
    *out = s;
    return NRSC5HIP_OK;
}

extern "C" void nrsc5hip_sis_destroy(nrsc5hip_sis *s) { sis_free(s); }

extern "C" int nrsc5hip_sis_reset(nrsc5hip_sis *s, int stream)
{
    if (!s || stream < 0 || stream >= s->nstreams) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream");
    nrsc5::DeviceGuard g(s->device);
    SisState st;
    sis_state_init(st);
    HIPCHK(hipMemcpy(s->state.p + stream, &st, sizeof(st), hipMemcpyHostToDevice));
    return NRSC5HIP_OK;
}

extern "C" int nrsc5hip_sis_debug_arena(nrsc5hip_sis *s, long long bytes)
{
    if (!s || bytes < 0) FAIL(NRSC5HIP_EINVAL, "bad consumer / size");
    s->arena_limit = bytes;
    return NRSC5HIP_OK;
}

extern "C" int nrsc5hip_sis_stats(nrsc5hip_sis *s, int stream, long long stats[NRSC5HIP_SIS_NSTATS])
{
    if (!s || !stats || stream < 0 || stream >= s->nstreams) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream");
    nrsc5::DeviceGuard g(s->device);
    return read_stats<SIS_STATS>(s->stats.p + (size_t)stream * SIS_STATS, s->ar.d2h, stats);
}

extern "C" int nrsc5hip_sis_get(nrsc5hip_sis *s, int stream, nrsc5hip_sis_info *out)
{
    if (!s || !out || stream < 0 || stream >= s->nstreams) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream");
    nrsc5::DeviceGuard g(s->device);
    SisState st;
    HIPCHK(hipMemcpy(&st, s->state.p + stream, sizeof(st), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));                               // report(), pids.c:284-383
    out->country_code[0] = (char)(st.cc & 0xff); out->country_code[1] = (char)((st.cc >> 8) & 0xff);
    out->fcc_facility_id = st.fcc;
    out->name_len = out->slogan_len = out->message_len = out->alert_len = out->alert_cnt_len = -1;
    auto cut = [](const uint8_t *p, int cap) { int n = 0; while (n < cap && p[n]) n++; return n; };
    if (st.usn_displayed) { out->name_enc = st.usn_enc; out->name_len = cut(st.usn_final, 15); memcpy(out->name, st.usn_final, (size_t)out->name_len); }
    else if (st.short_name[0]) { out->name_len = cut(st.short_name, 7); memcpy(out->name, st.short_name, (size_t)out->name_len); }
    // A frame 0 with the same seq rewrites a length while the item stays displayed (pids.c:540-543, 814-816, 872-875), and nothing checks it then:
    // the reference's report() reads past its arrays.  The snapshot shows what the buffers can hold: 190 / 95 / 381 bytes, control data within the alert.
    const int slogan_len = std::min(st.slogan_len, 95), msg_len = std::min(st.msg_len, 190), alert_len = std::min(st.alert_len, 381);
    const int cnt_len = std::min(st.alert_cnt_len, alert_len);
    if (st.slogan_displayed) { out->slogan_enc = st.slogan_enc; out->slogan_len = slogan_len; memcpy(out->slogan, st.slogan, (size_t)slogan_len); }
    else if (st.long_displayed) { out->slogan_len = cut(st.long_name, 56); memcpy(out->slogan, st.long_name, (size_t)out->slogan_len); }
    if (st.msg_displayed) { out->message_enc = st.msg_enc; out->message_len = msg_len; memcpy(out->message, st.message, (size_t)msg_len); }
    if (st.alert_displayed) { out->alert_enc = st.alert_enc; out->alert_len = alert_len; out->alert_cnt_len = cnt_len; memcpy(out->alert, st.alert, (size_t)alert_len); }
    if (st.have_lat && st.have_lon) { out->have_location = 1; out->latitude = st.lat; out->longitude = st.lon; out->altitude = st.altitude; }
    for (int i = 0; i < 8; i++)
        if (st.asd[i][1] != -1) { int32_t *a = out->audio[out->n_audio++]; a[0] = i; a[1] = st.asd[i][0]; a[2] = st.asd[i][1]; a[3] = st.asd[i][2]; }
    for (int i = 0; i < 16; i++)
        if (st.dsd[i][1] != -1) { int32_t *d = out->data[out->n_data++]; d[0] = st.dsd[i][0]; d[1] = st.dsd[i][1]; d[2] = st.dsd[i][2]; }
    return NRSC5HIP_OK;
}

// The device work of one call and the delivery.  frame_of[k]: the frame index, within its stream's list, that entry k of `entries` reports as
// (a reset-only entry never fires).  Nothing has been touched when this fails in front of the launch.
static int sis_run(nrsc5hip_sis *s, std::vector<ArenaStream> &streams, const std::vector<SisFrame> &entries, const std::vector<int> &frame_of,
                   nrsc5hip_sis_cb cb, void *opaque)
{
    const size_t ns = streams.size();
    if (ns == 0 || entries.empty()) return 0;
    // the arena, from what the host knows: a payload fires at most one event and adds at most 7 text bytes to what a later event can carry, a
    // frame has two payloads and may time the alert out; what the states hold already (56 + 190 + 15 + 95 + 381 bytes of text) can fire once
    size_t bound = 0;
    for (const ArenaStream &st : streams) bound += (size_t)st.count * 3 * (sizeof(SisEvent) + 8) + 5 * sizeof(SisEvent) + 1024;
    if (bound > 0xfffffff0u) FAIL(NRSC5HIP_EINVAL, "too many frames for one call");
    const size_t arena_cap = s->arena_limit ? std::min<size_t>(bound, (size_t)s->arena_limit) : bound;
    auto launch = [&](const ArenaDev &d) {
        SisArgs a;
        a.streams = d.streams; a.frames = (const SisFrame *)d.jobs; a.nentries = (int)entries.size();
        a.state = s->state.p; a.stats = s->stats.p; a.nstreams = s->nstreams;
        a.hdr = d.hdr; a.arena = d.arena; a.arena_cap = d.cap;
        launch_sis(a, (int)ns, nullptr);
    };
    return arena_round<SisEvent>(s->ar, nullptr, "event", "k_sis", streams, entries.data(), entries.size() * sizeof(SisFrame), arena_cap, launch,
                                 [&](const SisEvent &ev) { return ev.entry < (unsigned)streams[ev.pos].count; },
                                 [&](const ArenaStream &st, const SisEvent &ev, const uint8_t *data) {
                                     if (cb) cb(opaque, st.target, frame_of[(size_t)st.first + ev.entry], ev.kind, ev.v, ev.enc, data, ev.len);
                                 });
}

extern "C" int nrsc5hip_sis_feed(nrsc5hip_sis *s, int nstreams, const int *targets, const nrsc5hip_record *const *records, const int *counts,
                                 nrsc5hip_sis_cb cb, void *opaque)
{
    if (!s || nstreams < 0) FAIL(NRSC5HIP_EINVAL, "bad consumer / stream count");
    if (nstreams == 0) return 0;
    if (!records || !counts) FAIL(NRSC5HIP_EINVAL, "null argument");
    nrsc5::DeviceGuard g(s->device);
    int rc = check_targets(s->nstreams, nstreams, targets); if (rc) return rc;
    size_t total = 0;
    for (int i = 0; i < nstreams; i++) {
        if (counts[i] < 0 || (counts[i] > 0 && !records[i])) FAIL(NRSC5HIP_EINVAL, "records of stream %d of the call missing", i);
        total += (size_t)counts[i];
    }
    if (total > (size_t)INT32_MAX / 4) FAIL(NRSC5HIP_EINVAL, "too many records for one call");
    std::vector<ArenaStream> streams;
    std::vector<SisFrame> entries;
    std::vector<int> frame_of;
    entries.reserve(total); frame_of.reserve(total);
    for (int i = 0; i < nstreams; i++) {
        const int first = (int)entries.size();
        int nf = 0;
        for (int k = 0; k < counts[i]; k++) {
            const nrsc5hip_record &r = records[i][k];
            const bool pids = (r.flags & NRSC5HIP_REC_PIDS) != 0, reset = (r.flags & NRSC5HIP_REC_TO_FINE) != 0;
            if (!pids && !reset) continue;
            SisFrame f;
            f.w[0] = pids ? r.pids[0] : 0u; f.w[1] = pids ? r.pids[1] : 0u; f.w[2] = pids ? r.pids[2] : 0u;
            f.flags = (reset ? 1u : 0u) | (pids ? 0u : 2u);
            entries.push_back(f);
            frame_of.push_back(nf);
            if (pids) nf++;
        }
        if ((int)entries.size() > first) streams.push_back(ArenaStream{targets ? targets[i] : i, first, (int)entries.size() - first, (int)streams.size()});
    }
    return sis_run(s, streams, entries, frame_of, cb, opaque);
}

extern "C" int nrsc5hip_stage_sis(nrsc5hip_sis *s, int nstreams, const int *targets, const uint8_t *const *frames, const int *nframes,
                                  const int *reset_at, nrsc5hip_sis_cb cb, void *opaque)
{
    if (!s || nstreams < 1 || !frames || !nframes) FAIL(NRSC5HIP_EINVAL, "bad argument");
    nrsc5::DeviceGuard g(s->device);
    int rc = check_targets(s->nstreams, nstreams, targets); if (rc) return rc;
    size_t total = 0;
    for (int i = 0; i < nstreams; i++) {
        if (nframes[i] < 0 || (nframes[i] > 0 && !frames[i])) FAIL(NRSC5HIP_EINVAL, "stream %d of the call: frames missing", i);
        if (reset_at && reset_at[i] > nframes[i]) FAIL(NRSC5HIP_EINVAL, "stream %d of the call: reset behind the end", i);
        total += (size_t)nframes[i] + 1;
    }
    if (total > (size_t)INT32_MAX / 4) FAIL(NRSC5HIP_EINVAL, "too many frames for one call");
    std::vector<ArenaStream> streams;
    std::vector<SisFrame> entries;
    std::vector<int> frame_of;
    for (int i = 0; i < nstreams; i++) {
        const int first = (int)entries.size(), rst = reset_at ? reset_at[i] : -1;
        for (int f = 0; f < nframes[i]; f++) {
            SisFrame e{{0u, 0u, 0u}, f == rst ? 1u : 0u};
            for (int k = 0; k < NRSC5HIP_PIDS_FRAME_BITS; k++) e.w[k >> 5] |= (uint32_t)(frames[i][(size_t)f * NRSC5HIP_PIDS_FRAME_BITS + k] & 1u) << (k & 31);
            entries.push_back(e);
            frame_of.push_back(f);
        }
        if (rst >= 0 && rst == nframes[i]) { entries.push_back(SisFrame{{0u, 0u, 0u}, 3u}); frame_of.push_back(nframes[i]); }   // as a REC_TO_FINE record without a frame
        if ((int)entries.size() > first) streams.push_back(ArenaStream{targets ? targets[i] : i, first, (int)entries.size() - first, (int)streams.size()});
    }
    return sis_run(s, streams, entries, frame_of, cb, opaque);
}
