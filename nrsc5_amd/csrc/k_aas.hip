// Data services on the device: output_aas_push (output.c:874-896) over the packet arena k_psd leaves in device memory -- port routing, the Station
// Information Guide (parse_sig, output.c:512-625), process_port and LOT file reassembly (output.c:684-872).  The packets never reach the host: the SIG
// table, LOT headers, complete files, stream / packet data and the PSD-port packets do.
// One wave64 workgroup per listed stream: it walks the headers of the packet arena (few packets per call: a serial walk, every lane the same header) and
// takes the records whose `pos` is its stream's, in order, so a stream's state has one writer.  Workgroups never wait for each other.
// State: the SIG table and the file descriptors (AasStream, AasFile) are loaded into LDS at the start and written back at the end; the 64 KB of every file
// stay in global memory.  One lane changes a descriptor, a barrier follows, every lane reads it: all control flow is wave-uniform.  File bytes this
// wave stored are read back only behind a barrier (the copy of a complete file).
// The wave works where the bytes are: the port lookup (128 components, two per lane, a ballot), the fragment store with its zero tail (a dword per
// lane), the name compare and the search for its first NUL (a byte per lane and ballots), the completeness test (popcounts over the 256-bit mask,
// a word per lane) and the copy of a complete file into the event arena (16, 8 or 4 bytes per lane and step, as source and destination are aligned).
// The SIG walk is serial (once per station): lane 0.
// Bounds: a record is taken only if it lies inside the used part of the packet arena; every SIG read is checked against the packet; seq < 256 and
// len <= 256 in front of the fragment store; a file slot index comes from a ballot over lanes < lot_files; an event is written only into room that
// arena_reserve granted.
#include <hip/hip_runtime.h>
#include "nrsc5hip.h"
#include "kernels.h"

namespace nrsc5 {

struct AasSmem {
    AasService services[AAS_SERVICES];
    AasFile files[AAS_MAX_FILES];
    uint32_t lru;
};
static_assert(sizeof(AasSmem) <= 48 * 1024, "static LDS of one workgroup");

struct AasWave {
    const AasArgs &a; AasSmem &sm; const ArenaStream s; uint8_t *data; const int lane;
    unsigned long long c[AAS_STATS];
};

__device__ inline void aas_words(uint32_t *dst, const uint32_t *src, unsigned nwords, int lane) { for (unsigned i = (unsigned)lane; i < nwords; i += 64u) dst[i] = src[i]; }

// n bytes, as wide as both pointers are aligned; wave-uniform
__device__ inline void aas_copy(uint8_t *dst, const uint8_t *src, unsigned n, int lane)
{
    const unsigned long long both = (unsigned long long)dst | (unsigned long long)src;
    unsigned done = 0;
    if (!(both & 15ull)) {
        const unsigned k = n >> 4;
        for (unsigned i = (unsigned)lane; i < k; i += 64u) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
        done = k << 4;
    } else if (!(both & 7ull)) {
        const unsigned k = n >> 3;
        for (unsigned i = (unsigned)lane; i < k; i += 64u) ((uint2 *)dst)[i] = ((const uint2 *)src)[i];
        done = k << 3;
    } else if (!(both & 3ull)) {
        const unsigned k = n >> 2;
        for (unsigned i = (unsigned)lane; i < k; i += 64u) ((uint32_t *)dst)[i] = ((const uint32_t *)src)[i];
        done = k << 2;
    }
    for (unsigned i = done + (unsigned)lane; i < n; i += 64u) dst[i] = src[i];
}

// an event header in the arena -> the offset of its data, or ARENA_FULL (nothing may be written then)
__device__ inline unsigned aas_emit(AasWave &w, unsigned kind, unsigned port, unsigned seq, const int32_t (&v)[8], unsigned len)
{
    const unsigned rec = (unsigned)sizeof(AasEvent) + ((len + 3u) & ~3u);
    unsigned at = 0;
    if (w.lane == 0) at = arena_reserve(w.a.hdr, w.a.arena_cap, rec);
    at = __shfl(at, 0);
    if (at == ARENA_FULL) return ARENA_FULL;
    if (w.lane == 0) {
        AasEvent e;
        e.pos = (uint32_t)w.s.pos; e.len = len; e.kind = (uint16_t)kind; e.port = (uint16_t)port; e.seq = seq;
        for (int k = 0; k < 8; k++) e.v[k] = v[k];
        *(AasEvent *)(w.a.arena + at) = e;
        atomicAdd(&w.a.hdr->count, 1u);
    }
    w.c[AAS_C_EVENTS]++;
    return at + (unsigned)sizeof(AasEvent);
}

// parse_sig, output.c:512-625; lane 0 walks, the table in LDS has been cleared
__device__ inline void aas_sig_walk(AasWave &w, const uint8_t *buf, unsigned len, int *truncated, int *zero_len)
{
    AasService *service = nullptr;
    unsigned p = 0;
    while (p < len) {
        const unsigned type = buf[p++];
        if ((type & 0xF0u) == 0x40u) {
            if (p + 2 > len) { *truncated = 1; return; }
            const unsigned number = buf[p] | (buf[p + 1] << 8);
            int idx = 0;
            for (; idx < AAS_SERVICES; idx++) {
                if (w.sm.services[idx].type == 0) break;
                if (w.sm.services[idx].number == number) {                // a duplicate: cleared and used again, output.c:540-546
                    uint32_t *z = (uint32_t *)&w.sm.services[idx];
                    for (unsigned k = 0; k < sizeof(AasService) / 4; k++) z[k] = 0;
                    break;
                }
            }
            if (idx == AAS_SERVICES) return;
            service = &w.sm.services[idx];
            service->type = type == 0x40u ? 2 : 1;
            service->number = (uint16_t)number;
            p += 3;
        } else if ((type & 0xF0u) == 0x60u) {
            if (p >= len) { *truncated = 1; return; }
            const unsigned l = buf[p++];
            if (!service) return;
            if (l == 0) { *zero_len = 1; return; }
            if (type == 0x69u) {
                if (l < 2 || p + 1 + (l - 2) > len) { *truncated = 1; return; }
                service->name_len = l - 2;
                for (unsigned k = 0; k < l - 2; k++) service->name[k] = buf[p + 1 + k];
            } else if (type == 0x67u || type == 0x66u) {
                const unsigned need = type == 0x67u ? 12u : 11u;
                if (p + need > len) { *truncated = 1; return; }
                const unsigned id = buf[p];
                int ci = 0;
                for (; ci < AAS_COMPONENTS; ci++) if (service->comp[ci].type == 0 || service->comp[ci].id == id) break;     // find_component
                if (ci == AAS_COMPONENTS) return;
                AasComponent c;
                c.id = (uint8_t)id; c.pad = 0;
                if (type == 0x67u) {
                    c.type = 1; c.port = (uint16_t)(buf[p + 1] | (buf[p + 2] << 8)); c.service_data_type = (uint16_t)(buf[p + 3] | (buf[p + 4] << 8));
                    c.data_type = buf[p + 5]; c.mime = buf[p + 8] | (buf[p + 9] << 8) | (buf[p + 10] << 16) | ((uint32_t)buf[p + 11] << 24);
                } else {
                    c.type = 2; c.port = buf[p + 1]; c.service_data_type = 0; c.data_type = buf[p + 2];
                    c.mime = buf[p + 7] | (buf[p + 8] << 8) | (buf[p + 9] << 16) | ((uint32_t)buf[p + 10] << 24);
                }
                service->comp[ci] = c;
            }
            p += l - 1;
        } else return;
    }
}

__device__ inline void aas_sig(AasWave &w, const uint8_t *buf, unsigned len)
{
    w.c[AAS_C_SIG]++;
    __syncthreads();
    if (w.sm.services[0].type != 0) return;                     // processed once, output.c:517-521
    __syncthreads();
    { uint32_t *z = (uint32_t *)w.sm.services; for (unsigned i = (unsigned)w.lane; i < sizeof(w.sm.services) / 4; i += 64u) z[i] = 0; }
    __syncthreads();
    int truncated = 0, zero_len = 0;
    if (w.lane == 0) aas_sig_walk(w, buf, len, &truncated, &zero_len);
    __syncthreads();
    truncated = __shfl(truncated, 0); zero_len = __shfl(zero_len, 0);
    w.c[AAS_C_SIG_PARSED]++; w.c[AAS_C_SIG_TRUNCATED] += (unsigned)truncated; w.c[AAS_C_SIG_ZERO_LEN] += (unsigned)zero_len;
    if (w.sm.services[0].type == 0) w.c[AAS_C_SIG_EMPTY]++;
    unsigned n = 0, ns = 0;
    if (w.lane == 0) n = aas_sig_flatten(w.sm.services, nullptr, &ns);
    n = __shfl(n, 0); ns = __shfl(ns, 0);
    const int32_t v[8] = {(int32_t)ns, 0, 0, 0, 0, 0, 0, 0};
    const unsigned at = aas_emit(w, NRSC5HIP_AAS_SIG, 0x20u, 0u, v, n);
    if (at != ARENA_FULL && w.lane == 0) (void)aas_sig_flatten(w.sm.services, w.a.arena + at, &ns);
}

// the part of process_port behind the type switch for NRSC5_AAS_TYPE_LOT, output.c:715-866
__device__ inline void aas_lot(AasWave &w, int comp, unsigned port, const uint8_t *buf, unsigned len)
{
    const int lane = w.lane, nf = w.a.lot_files;
    w.c[AAS_C_LOT_PACKETS]++;
    if (len < 8u) { w.c[AAS_C_LOT_BAD]++; return; }
    unsigned hdrlen = buf[0];
    const unsigned repeat = buf[1], lot = buf[2] | (buf[3] << 8), seq = buf[4] | (buf[5] << 8) | (buf[6] << 16) | ((uint32_t)buf[7] << 24);
    if (hdrlen < 8u || hdrlen > len) { w.c[AAS_C_LOT_BAD]++; return; }
    buf += 8; len -= 8u; hdrlen -= 8u;
    if (seq >= (unsigned)AAS_FRAGMENTS) { w.c[AAS_C_LOT_BAD]++; return; }

    __syncthreads();
    const bool mine = lane < nf;
    const uint32_t ts = mine ? w.sm.files[lane].timestamp : 0u;
    const bool live = mine && ts != 0u && w.sm.files[lane].owner == comp;
    const int local = live ? w.sm.files[lane].local : -1;
    const unsigned long long found = __ballot(live && w.sm.files[lane].lot == lot);          // find_lot
    int slot;
    if (found) slot = __builtin_ctzll(found);
    else {                                                      // find_free_lot, then a slot of the stream's pool for it
        unsigned used = 0;
        for (int k = 0; k < AAS_LOT_PER_COMPONENT; k++) if (__ballot(local == k)) used |= 1u << k;
        int at_local;
        if (used != (1u << AAS_LOT_PER_COMPONENT) - 1u) {
            at_local = __builtin_ctz(~used);
            const unsigned long long free_slots = __ballot(mine && ts == 0u);
            if (free_slots) slot = __builtin_ctzll(free_slots);
            else {                                              // the pool is full: the stream's least recently stamped file goes
                unsigned long long key = mine ? ((unsigned long long)ts << 8) | (unsigned)lane : ~0ull;
                for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(key, d); key = o < key ? o : key; }
                slot = (int)(key & 0xffull);
                w.c[AAS_C_POOL_EVICTIONS]++;
            }
        } else {                                                // the component's least recently used of 12; the first of equals in its array
            unsigned long long key = live ? ((unsigned long long)ts << 16) | ((unsigned)local << 8) | (unsigned)lane : ~0ull;
            for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(key, d); key = o < key ? o : key; }
            slot = (int)(key & 0xffull); at_local = (int)((key >> 8) & 0xffull);
            w.c[AAS_C_LRU_EVICTIONS]++;
        }
        __syncthreads();
        { uint32_t *z = (uint32_t *)&w.sm.files[slot]; for (unsigned i = (unsigned)lane; i < sizeof(AasFile) / 4; i += 64u) z[i] = 0; }
        __syncthreads();
        if (lane == 0) { w.sm.files[slot].owner = comp; w.sm.files[slot].local = at_local; w.sm.files[slot].lot = lot; }
    }
    AasFile &f = w.sm.files[slot];
    __syncthreads();
    if (lane == 0) f.timestamp = w.sm.lru++;                    // before the header is looked at, output.c:748
    __syncthreads();

    int new_data = 0;
    if (hdrlen > 0u) {
        if (hdrlen < 16u) { w.c[AAS_C_LOT_SHORT_HEADER]++; return; }
        int32_t exp[5];
        exp[0] = (int32_t)((buf[7] << 4) | (buf[6] >> 4)) - 1900; exp[1] = (int32_t)(buf[6] & 0xfu) - 1; exp[2] = (int32_t)(buf[5] >> 3);
        exp[3] = (int32_t)(((buf[5] & 0x7u) << 2) | (buf[4] >> 6)); exp[4] = (int32_t)(buf[4] & 0x3fu);
        const uint32_t size = buf[8] | (buf[9] << 8) | (buf[10] << 16) | ((uint32_t)buf[11] << 24);
        const uint32_t mime = buf[12] | (buf[13] << 8) | (buf[14] << 16) | ((uint32_t)buf[15] << 24);
        buf += 16; len -= 16u; hdrlen -= 16u;                   // what is left of the header is the name
        // the name as strndup keeps it: cut at its first NUL
        unsigned kept = hdrlen;
        bool differs = false;
        for (unsigned base = 0; base < hdrlen; base += 64u) {
            const unsigned i = base + (unsigned)lane;
            const bool valid = i < hdrlen;
            const unsigned b = valid ? buf[i] : 1u;
            const unsigned long long z = __ballot(valid && b == 0u);
            if (z && kept == hdrlen) kept = base + (unsigned)__builtin_ctzll(z);
            if (__ballot(valid && b != f.name[i])) differs = true;
        }
        if (f.has_name) {
            bool changed = hdrlen != f.name_len || differs || size != f.size || mime != f.mime;
            for (int k = 0; k < 5; k++) changed = changed || exp[k] != f.expiry[k];
            if (changed) {                                      // the metadata has changed: the file starts over, output.c:788-795
                const int keep_local = f.local;
                __syncthreads();
                { uint32_t *z = (uint32_t *)&f; for (unsigned i = (unsigned)lane; i < sizeof(AasFile) / 4; i += 64u) z[i] = 0; }
                __syncthreads();
                if (lane == 0) { f.owner = comp; f.local = keep_local; f.lot = lot; f.timestamp = w.sm.lru; }
                w.c[AAS_C_LOT_RESETS]++;
                new_data = 1;
            }
        } else new_data = 1;
        __syncthreads();
        for (unsigned i = (unsigned)lane; i < hdrlen; i += 64u) f.name[i] = buf[i];
        if (lane == 0) { f.has_name = 1; f.name_len = kept; f.size = size; f.mime = mime; for (int k = 0; k < 5; k++) f.expiry[k] = exp[k]; }
        __syncthreads();
        buf += hdrlen; len -= hdrlen;
        if (new_data) {
            const int32_t v[8] = {(int32_t)lot, (int32_t)size, (int32_t)mime, exp[0], exp[1], exp[2], exp[3], exp[4]};
            const unsigned at = aas_emit(w, NRSC5HIP_AAS_LOT_HEADER, port, 0u, v, kept);
            if (at != ARENA_FULL) for (unsigned i = (unsigned)lane; i < kept; i += 64u) w.a.arena[at + i] = f.name[i];
            w.c[AAS_C_LOT_HEADERS]++;
        }
    }

    uint8_t *fdata = w.data + (size_t)slot * AAS_FILE_BYTES;
    const int dup = (f.mask[seq >> 5] >> (seq & 31u)) & 1u;
    if (!dup) {
        new_data = 1;
        if (len > (unsigned)AAS_FRAGMENT) { w.c[AAS_C_LOT_TOO_LARGE]++; return; }          // neither stored nor reported, output.c:831-835
        uint32_t word = 0;                                      // the fragment and its zero tail: a dword per lane
        for (unsigned k = 0; k < 4u; k++) { const unsigned i = 4u * (unsigned)lane + k; if (i < len) word |= (uint32_t)buf[i] << (8u * k); }
        ((uint32_t *)(fdata + seq * (unsigned)AAS_FRAGMENT))[lane] = word;
        __syncthreads();
        if (lane == 0) { f.mask[seq >> 5] |= 1u << (seq & 31u); f.bytes_so_far += len; }
        __syncthreads();
    } else w.c[AAS_C_LOT_DUPLICATES]++;
    w.c[AAS_C_LOT_FRAGMENTS]++;
    if (w.a.flags & AAS_FLAG_FRAGMENTS) {
        const int32_t v[8] = {(int32_t)lot, (int32_t)repeat, dup, (int32_t)len, (int32_t)f.bytes_so_far, 0, 0, 0};
        (void)aas_emit(w, NRSC5HIP_AAS_LOT_FRAGMENT, port, seq, v, 0u);
    }

    const uint32_t size = f.size;
    if (!new_data || size == 0u) return;
    if (size > (uint32_t)AAS_FILE_BYTES) { w.c[AAS_C_LOT_OVERSIZE]++; return; }
    const unsigned nfrag = (size + (unsigned)AAS_FRAGMENT - 1u) / (unsigned)AAS_FRAGMENT;
    bool missing = false;
    if (lane < AAS_FRAGMENTS / 32) {
        const unsigned lo = 32u * (unsigned)lane;
        const uint32_t need = nfrag >= lo + 32u ? 0xffffffffu : nfrag > lo ? (1u << (nfrag - lo)) - 1u : 0u;
        missing = __popc(f.mask[lane] & need) != __popc(need);
    }
    if (__ballot(missing)) return;
    const unsigned name_len = f.name_len;
    const int32_t v[8] = {(int32_t)lot, (int32_t)size, (int32_t)f.mime, f.expiry[0], f.expiry[1], f.expiry[2], f.expiry[3], f.expiry[4]};
    const unsigned at = aas_emit(w, NRSC5HIP_AAS_LOT, port, name_len, v, size + name_len);
    w.c[AAS_C_LOT_FILES]++;
    if (at == ARENA_FULL) return;
    __syncthreads();                                            // behind this wave's fragment stores
    aas_copy(w.a.arena + at, fdata, size, lane);
    for (unsigned i = (unsigned)lane; i < name_len; i += 64u) w.a.arena[at + size + i] = f.name[i];
}

// process_port, output.c:684-872
__device__ inline void aas_port(AasWave &w, unsigned port, unsigned seq, const uint8_t *buf, unsigned len)
{
    __syncthreads();
    if (w.sm.services[0].type == 0) { w.c[AAS_C_BEFORE_SIG]++; return; }
    // find_port: the first data component with this port, in service order -- components lane and lane + 64
    const AasComponent &c0 = w.sm.services[w.lane >> 3].comp[w.lane & 7], &c1 = w.sm.services[8 + (w.lane >> 3)].comp[w.lane & 7];
    const unsigned long long m0 = __ballot(c0.type == 1 && c0.port == port), m1 = __ballot(c1.type == 1 && c1.port == port);
    if (!m0 && !m1) { w.c[AAS_C_NOT_IN_SIG]++; return; }
    const int comp = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1);
    const AasComponent c = w.sm.services[comp >> 3].comp[comp & 7];
    if (c.data_type == 0 || c.data_type == 1) {                 // NRSC5_AAS_TYPE_STREAM, _PACKET
        const int32_t v[8] = {(int32_t)c.mime, comp >> 3, comp & 7, 0, 0, 0, 0, 0};
        const unsigned at = aas_emit(w, c.data_type == 0 ? NRSC5HIP_AAS_STREAM : NRSC5HIP_AAS_PACKET, port, seq, v, len);
        if (at != ARENA_FULL) aas_copy(w.a.arena + at, buf, len, w.lane);
        w.c[c.data_type == 0 ? AAS_C_STREAM : AAS_C_PACKET]++;
    } else if (c.data_type == 3) aas_lot(w, comp, port, buf, len);
    else w.c[AAS_C_UNKNOWN_TYPE]++;
}

__global__ __launch_bounds__(64) void k_aas(AasArgs a)
{
    __shared__ AasSmem sm;
    const int lane = (int)threadIdx.x;
    const ArenaStream s = a.streams[blockIdx.x];
    if (s.target < 0 || s.target >= a.nstreams || a.lot_files < 1 || a.lot_files > AAS_MAX_FILES) return;
    const unsigned in_used = a.in_hdr->used;
    if (a.in_hdr->overflow || in_used > a.in_cap) {             // the packets of this call are lost: the host reports it
        if (lane == 0) atomicOr(&a.hdr->overflow, 2u);
        return;
    }
    AasStream *gst = a.state + s.target;
    AasFile *gfiles = a.files + (size_t)s.target * a.lot_files;
    aas_words((uint32_t *)sm.services, (const uint32_t *)gst->services, (unsigned)sizeof(sm.services) / 4u, lane);
    aas_words((uint32_t *)sm.files, (const uint32_t *)gfiles, (unsigned)(a.lot_files * sizeof(AasFile)) / 4u, lane);
    if (lane == 0) sm.lru = gst->lot_lru_counter;
    __syncthreads();
    AasWave w{a, sm, s, a.data + (size_t)s.target * a.lot_files * AAS_FILE_BYTES, lane, {}};
    for (int k = 0; k < AAS_STATS; k++) w.c[k] = 0;

    for (unsigned at = 0; at + (unsigned)sizeof(PsdPacket) <= in_used;) {
        const PsdPacket p = *(const PsdPacket *)(a.in_arena + at);
        const unsigned rec = (unsigned)sizeof(PsdPacket) + (((unsigned)p.len + 3u) & ~3u);
        if (rec > in_used - at) break;
        const uint8_t *buf = a.in_arena + at + sizeof(PsdPacket);
        at += rec;
        if (p.pos != (uint32_t)s.pos) continue;
        w.c[AAS_C_PACKETS]++;
        const unsigned port = p.port, len = p.len;
        if (port == 0x5100u || (port >= 0x5201u && port <= 0x5207u)) {                     // output.c:878-882: to the host as it is
            const int32_t v[8] = {(int32_t)p.program, 0, 0, 0, 0, 0, 0, 0};
            const unsigned out = aas_emit(w, NRSC5HIP_AAS_PSD, port, p.seq, v, len);
            if (out != ARENA_FULL) aas_copy(a.arena + out, buf, len, lane);
            w.c[AAS_C_PSD]++;
        } else if (port == 0x20u) aas_sig(w, buf, len);
        else if (port >= 0x401u && port <= 0x50FFu) aas_port(w, port, p.seq, buf, len);
        else w.c[AAS_C_UNKNOWN_PORT]++;
    }

    __syncthreads();
    aas_words((uint32_t *)gst->services, (const uint32_t *)sm.services, (unsigned)sizeof(sm.services) / 4u, lane);
    aas_words((uint32_t *)gfiles, (const uint32_t *)sm.files, (unsigned)(a.lot_files * sizeof(AasFile)) / 4u, lane);
    if (lane == 0) {
        gst->lot_lru_counter = sm.lru;
        unsigned long long *st = a.stats + (size_t)s.target * AAS_STATS;
        for (int k = 0; k < AAS_STATS; k++) st[k] += w.c[k];
    }
}

void launch_aas(const AasArgs &a, int nstreams, hipStream_t st)
{
    if (nstreams < 1) return;
    hipLaunchKernelGGL(k_aas, dim3(nstreams), dim3(64), 0, st, a);
}

}  // namespace nrsc5
