// race_state_api.hip -- C ABI of the race's snapshot, restore and clone (include/lpvmpc.h, "Race snapshot, restore and clone").
// All three walk one table, the inventory of the race's per-vehicle state that lpvmpc_race_state (race_api.hip) fills for the
// running race: snapshot copies every array of it to the host behind a self-describing header, restore copies a blob whose header
// and directory equal the live race's back, clone moves vehicles' words within the arrays (kernels: race_state.hip).  None of
// them is on a tick's path; the clone's staging buffer is a local arena, released when the call returns.
#include <algorithm>
#include <cstring>

#include "lpvmpc_handle.hpp"
#include "race_state.hpp"

namespace {

constexpr char kMagic[8] = {'L', 'P', 'V', 'R', 'A', 'C', 'E', '\0'};
constexpr int kHeaderBytes = LPVMPC_SNAP_HEADER_BYTES, kEntryBytes = LPVMPC_SNAP_ENTRY_BYTES;
constexpr int kShapeWords = 8;                  // B, N, Np, M, sd, lap_cols, laps, ticks
const char *const kShapeNames[kShapeWords] = {"B", "N", "Np", "M", "sd", "lap_cols", "laps", "ticks"};

size_t elem_bytes(int type) { return type == lpvmpc::STATE_I32 ? 4 : 8; }
size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }
size_t array_bytes(const RaceStateDesc &e, size_t B) { return B * (size_t)e.W * elem_bytes(e.type); }

// byte offset of every array in the blob and the blob's size
size_t blob_layout(const RaceState &s, std::vector<size_t> &off) {
    size_t at = (size_t)kHeaderBytes + (size_t)kEntryBytes * s.tab.size();
    off.clear();
    for (const RaceStateDesc &e : s.tab) { off.push_back(at); at += align8(array_bytes(e, (size_t)s.shape[0])); }
    return at;
}

// little-endian words at p (gfx950's hosts are little-endian: plain copies)
void put32(char *p, int32_t v) { std::memcpy(p, &v, 4); }
void put64(char *p, int64_t v) { std::memcpy(p, &v, 8); }
int32_t get32(const char *p) { int32_t v; std::memcpy(&v, p, 4); return v; }
int64_t get64(const char *p) { int64_t v; std::memcpy(&v, p, 8); return v; }

}  // namespace

extern "C" int lpvmpc_race_snapshot_size(lpvmpc_handle *h, int64_t *bytes) {
    RaceState s;
    if (!h || !lpvmpc_race_state(h, s)) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_snapshot_size: call lpvmpc_race_init first");
    if (!bytes) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_snapshot_size: bytes is NULL");
    std::vector<size_t> off;
    bytes[0] = (int64_t)blob_layout(s, off);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_snapshot(lpvmpc_handle *h, void *buf, int64_t bytes) {
    RaceState s;
    if (!h || !lpvmpc_race_state(h, s)) return fail(h, LPVMPC_E_ARG, "lpvmpc_race_snapshot: call lpvmpc_race_init first");
    std::vector<size_t> off;
    const size_t need = blob_layout(s, off);
    if (!buf || bytes < 0 || (size_t)bytes < need)
        return fail(h, LPVMPC_E_ARG, "lpvmpc_race_snapshot: the buffer is NULL or holds %lld B, the snapshot needs %zu B (lpvmpc_race_snapshot_size)",
                    (long long)bytes, need);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));
    char *out = (char *)buf;
    std::memset(out, 0, (size_t)kHeaderBytes + (size_t)kEntryBytes * s.tab.size());
    std::memcpy(out, kMagic, 8);
    put32(out + 8, LPVMPC_SNAP_VERSION);
    for (int i = 0; i < kShapeWords; ++i) put32(out + 12 + 4 * i, s.shape[i]);
    put32(out + 44, (int32_t)s.features);
    put32(out + 48, (int32_t)s.tab.size());
    for (size_t i = 0; i < s.tab.size(); ++i) {
        const RaceStateDesc &e = s.tab[i];
        char *d = out + kHeaderBytes + kEntryBytes * i;
        std::memcpy(d, e.name, 16);
        put32(d + 16, e.type); put32(d + 20, e.W); put32(d + 24, e.layout);
        put64(d + 32, (int64_t)off[i]);
        const size_t n = array_bytes(e, (size_t)s.shape[0]);
        if (align8(n) != n) std::memset(out + off[i] + n, 0, align8(n) - n);      // the padding behind an odd i32 array
        D2H(out + off[i], e.ptr, n);
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_restore(lpvmpc_handle *h, const void *buf, int64_t bytes) {
    const char *who = "lpvmpc_race_restore";
    RaceState s;
    if (!h || !lpvmpc_race_state(h, s)) return fail(h, LPVMPC_E_ARG, "%s: call lpvmpc_race_init first", who);
    if (s.recording)
        return fail(h, LPVMPC_E_ARG, "%s: a recorder is attached, and its ring and statistics do not travel with the state; stop it first "
                    "(lpvmpc_race_record with capacity 0)", who);
    if (s.heats)
        return fail(h, LPVMPC_E_ARG, "%s: heats are attached, and a position history means nothing after a restore; detach them first "
                    "(lpvmpc_race_heats(path, cfg, NULL, NULL))", who);
    if (s.events)
        return fail(h, LPVMPC_E_ARG, "%s: an event log is attached, and before and after mean nothing across a restore; detach it first "
                    "(lpvmpc_race_events(path, NULL))", who);
    if (!buf || bytes < kHeaderBytes) return fail(h, LPVMPC_E_ARG, "%s: the buffer is NULL or shorter than the %d B header (%lld B)", who, kHeaderBytes, (long long)bytes);
    const char *in = (const char *)buf;
    if (std::memcmp(in, kMagic, 8) != 0) return fail(h, LPVMPC_E_ARG, "%s: not a race snapshot (magic)", who);
    if (get32(in + 8) != LPVMPC_SNAP_VERSION) return fail(h, LPVMPC_E_ARG, "%s: snapshot format version %d, this library reads version %d", who, get32(in + 8), LPVMPC_SNAP_VERSION);
    for (int i = 0; i < kShapeWords - 1; ++i)                                   // (ticks is state: the last shape word is taken, not compared)
        if (get32(in + 12 + 4 * i) != s.shape[i])
            return fail(h, LPVMPC_E_ARG, "%s: the snapshot's %s = %d, the race's %d", who, kShapeNames[i], get32(in + 12 + 4 * i), s.shape[i]);
    const int32_t ticks = get32(in + 12 + 4 * (kShapeWords - 1));
    if (ticks < 0) return fail(h, LPVMPC_E_ARG, "%s: the snapshot's ticks = %d", who, ticks);
    if ((uint32_t)get32(in + 44) != s.features)
        return fail(h, LPVMPC_E_ARG, "%s: the snapshot's feature word 0x%x (estimator 1, actuator 2, disturbances 4, tracks 8, tyre wear 16), the race's 0x%x", who,
                    (unsigned)get32(in + 44), s.features);
    if (get32(in + 48) != (int32_t)s.tab.size())
        return fail(h, LPVMPC_E_ARG, "%s: the snapshot holds %d arrays, the race's state %zu", who, get32(in + 48), s.tab.size());
    std::vector<size_t> off;
    const size_t need = blob_layout(s, off);
    if ((size_t)bytes < need) return fail(h, LPVMPC_E_ARG, "%s: the buffer is truncated: %lld B of %zu B", who, (long long)bytes, need);
    for (size_t i = 0; i < s.tab.size(); ++i) {
        const RaceStateDesc &e = s.tab[i];
        const char *d = in + kHeaderBytes + kEntryBytes * i;
        char name[17] = {0};
        std::memcpy(name, d, 16);
        if (std::memcmp(d, e.name, 16) != 0) return fail(h, LPVMPC_E_ARG, "%s: array %zu of the snapshot is \"%s\", of the race's state \"%s\"", who, i, name, e.name);
        if (get32(d + 16) != e.type || get32(d + 20) != e.W || get32(d + 24) != e.layout)
            return fail(h, LPVMPC_E_ARG, "%s: array \"%s\": the snapshot's (type, W, layout) = (%d, %d, %d), the race's (%d, %d, %d)", who, e.name,
                        get32(d + 16), get32(d + 20), get32(d + 24), e.type, e.W, e.layout);
        if (get64(d + 32) != (int64_t)off[i])
            return fail(h, LPVMPC_E_ARG, "%s: array \"%s\": the snapshot's offset %lld, expected %zu", who, e.name, (long long)get64(d + 32), off[i]);
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));                                       // no tick in flight writes behind the copies
    for (size_t i = 0; i < s.tab.size(); ++i) H2D(s.tab[i].ptr, in + off[i], array_bytes(s.tab[i], (size_t)s.shape[0]));
    HIP_TRY(h, hipStreamSynchronize(st));
    lpvmpc_race_set_ticks(h, ticks);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_clone(lpvmpc_handle *h, const int32_t *src, int32_t *moved_out) {
    const char *who = "lpvmpc_race_clone";
    RaceState s;
    if (!h || !lpvmpc_race_state(h, s)) return fail(h, LPVMPC_E_ARG, "%s: call lpvmpc_race_init first", who);
    if (s.recording)
        return fail(h, LPVMPC_E_ARG, "%s: a recorder is attached, and its per-vehicle statistics do not move with the state; stop it first "
                    "(lpvmpc_race_record with capacity 0)", who);
    if (s.heats)
        return fail(h, LPVMPC_E_ARG, "%s: heats are attached, and their standings do not move with the state; detach them first "
                    "(lpvmpc_race_heats(path, cfg, NULL, NULL))", who);
    if (s.events)
        return fail(h, LPVMPC_E_ARG, "%s: an event log is attached, and its before words do not move with the state; detach it first "
                    "(lpvmpc_race_events(path, NULL))", who);
    if (!src) return fail(h, LPVMPC_E_ARG, "%s: src is NULL", who);
    const int B = s.shape[0];
    std::vector<int32_t> srcv, dstv;
    for (int b = 0; b < B; ++b) {
        if (src[b] < 0 || src[b] >= B) return fail(h, LPVMPC_E_ARG, "%s: src[%d] = %d is outside [0, %d)", who, b, src[b], B);
        if (s.track_of && (*s.track_of)[src[b]] != (*s.track_of)[b])
            return fail(h, LPVMPC_E_ARG, "%s: src[%d] = %d is on track %d, vehicle %d on track %d: a pose and a lap table mean nothing on another track",
                        who, b, src[b], (*s.track_of)[src[b]], b, (*s.track_of)[b]);
        if (src[b] != b) { srcv.push_back(src[b]); dstv.push_back(b); }
    }
    const size_t moved = dstv.size();
    if (moved_out) moved_out[0] = (int32_t)moved;
    if (moved == 0) return LPVMPC_OK;
    // the device table and the stage: each array's moved words in its own layout
    std::vector<lpvmpc::StateDescDev> tab(s.tab.size());
    size_t stage_bytes = 0, max_words = 0;
    for (size_t i = 0; i < tab.size(); ++i) {
        const RaceStateDesc &e = s.tab[i];
        tab[i] = lpvmpc::StateDescDev{e.ptr, (unsigned long long)stage_bytes, e.type, e.W, e.layout, 0};
        stage_bytes += align8(moved * (size_t)e.W * elem_bytes(e.type));
        max_words = std::max(max_words, moved * (size_t)e.W);
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    DevArena mem;                                                               // local: the call synchronises before it returns
    lpvmpc::StateDescDev *d_tab = nullptr;
    int32_t *d_src = nullptr, *d_dst = nullptr;
    char *d_stage = nullptr;
    hipError_t err = mem.alloc(d_tab, tab.size() * sizeof(tab[0]));
    if (err == hipSuccess) err = mem.alloc(d_src, moved * 4);
    if (err == hipSuccess) err = mem.alloc(d_dst, moved * 4);
    if (err == hipSuccess) err = mem.alloc(d_stage, stage_bytes);
    if (err != hipSuccess) return fail(h, LPVMPC_E_NOMEM, "%s: hipMalloc of the staging buffer (%zu B) failed: %s", who, stage_bytes, hipGetErrorString(err));
    err = hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(tab[0]), hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipMemcpyAsync(d_src, srcv.data(), moved * 4, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipMemcpyAsync(d_dst, dstv.data(), moved * 4, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = lpvmpc::launch_race_gather(d_tab, (int)tab.size(), B, (int)moved, d_src, d_stage, max_words, st);
    if (err == hipSuccess) err = lpvmpc::launch_race_scatter(d_tab, (int)tab.size(), B, (int)moved, d_dst, d_stage, max_words, st);
    const hipError_t serr = hipStreamSynchronize(st);                           // before the arena and the host vectors go
    if (err == hipSuccess) err = serr;
    if (err != hipSuccess) return fail(h, LPVMPC_E_HIP, "%s: %s", who, hipGetErrorString(err));
    return LPVMPC_OK;
}
