// events_api.hip -- C ABI of the race event log (include/lpvmpc.h, "Race event log"): attaching it to a race, reading the ring, and the
// stand-alone tick on caller-supplied data.  Kernels: events.hip.  The binding lives in the race (race_api.hip owns the slot and
// launches the tick's kernel last, behind the heats'); it is built in a local and installed only when it is whole.
#include <algorithm>
#include <new>
#include <vector>

#include "events_host.hpp"
#include "heats_host.hpp"

namespace {

bool mul_size(size_t &acc, size_t x) { return !__builtin_mul_overflow(acc, x, &acc); }

int check_kinds(lpvmpc_handle *h, const char *who, uint32_t kinds) {
    if (kinds & ~LPVMPC_EVENT_ALL_KINDS) return fail(h, LPVMPC_E_ARG, "%s: kinds = 0x%x has a bit outside 1 .. 8", who, kinds);
    return LPVMPC_OK;
}

}  // namespace

extern "C" void lpvmpc_event_default_config(lpvmpc_event_config *c) {
    if (!c) return;
    c->capacity = 65536; c->kinds = LPVMPC_EVENT_ALL_KINDS; c->reserved[0] = c->reserved[1] = 0;
}

extern "C" int lpvmpc_race_events(lpvmpc_handle *h, const lpvmpc_event_config *cfg) {
    const char *who = "lpvmpc_race_events";
    RaceAttach a;
    RC_TRY(a.begin(h, who));
    const RaceAttachView &v = a.v;
    hipStream_t st = a.st;
    if (!cfg) return lpvmpc_race_detach(h, RACE_EVENTS);
    if (cfg->capacity < 1) return fail(h, LPVMPC_E_ARG, "%s: capacity = %d must be >= 1", who, cfg->capacity);
    RC_TRY(check_kinds(h, who, cfg->kinds));
    if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
        return fail(h, LPVMPC_E_ARG, "%s: reserved = {%d, %d} must be 0", who, cfg->reserved[0], cfg->reserved[1]);
    const size_t B = v.B, cap = cfg->capacity;
    size_t ni = cap, nf = cap, nc = B;
    if (!mul_size(ni, LPVMPC_EVENT_I32 * sizeof(int32_t)) || !mul_size(nf, LPVMPC_EVENT_F64 * sizeof(double)) ||
        !mul_size(nc, LPVMPC_EVENT_CARRY_I32 * sizeof(int32_t)))
        return fail(h, LPVMPC_E_ARG, "%s: capacity %d overflows the buffer size", who, cfg->capacity);
    std::unique_ptr<EventBinding> q(new (std::nothrow) EventBinding());          // installed once it is complete
    if (!q) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    lpvmpc::EventDev &e = q->d;
    const Planes pl = lpvmpc_event_planes(e, B);
    DevTake take{q->mem};
    pl.alloc(take);
    take(e.ev_i, ni); take(e.ev_f, nf); take(e.total, 8); take(q->heat_of, B * 4);
    RC_TRY(take.check(h, who, true));
    e.B = v.B; e.kinds = cfg->kinds; e.capacity = cfg->capacity; e.n_events = nullptr;
    q->cfg = *cfg;
    return lpvmpc_race_install(h, st, *v.events, q, [&]() -> int {             // (its synchronisation: no tick in flight reads the old binding)
        RC_TRY(pl.blank_carry(h, st, nullptr));                                 // all zero: just attached
        HIP_TRY(h, hipMemsetAsync(e.out_i, 0, pl.out_i_bytes(), st));
        HIP_TRY(h, hipMemsetAsync(e.total, 0, 8, st));
        HIP_TRY(h, hipMemsetAsync(q->heat_of, 0xff, B * 4, st));
        return LPVMPC_OK;
    });
}

extern "C" int lpvmpc_race_events_read(lpvmpc_handle *h, int32_t n, int64_t *total, int32_t *kept, int32_t *i32, double *f64, int32_t *out_i32) {
    const char *who = "lpvmpc_race_events_read";
    RaceAttach a;
    RC_TRY(a.begin(h, who));
    EventBinding *q = a.v.events->get();
    if (!q) return fail(h, LPVMPC_E_ARG, "%s: no event log is attached (lpvmpc_race_events)", who);
    if (n < 0) return fail(h, LPVMPC_E_ARG, "%s: n < 0", who);
    hipStream_t st = a.st;
    unsigned long long tot = 0;
    D2H(&tot, q->d.total, 8);
    HIP_TRY(h, hipStreamSynchronize(st));                                       // the copies' sizes are in the count
    const unsigned long long cap = (unsigned long long)q->d.capacity;
    const unsigned long long k = tot < cap ? tot : cap, m = (unsigned long long)n < k ? (unsigned long long)n : k;
    const unsigned long long g0 = tot - m;                                      // the first event copied (0-based since the attach)
    for (unsigned long long j = 0; j < m;) {                                    // at most two runs of the ring
        const unsigned long long slot = (g0 + j) % cap, run = std::min(m - j, cap - slot);
        if (i32) D2H(i32 + j * LPVMPC_EVENT_I32, q->d.ev_i + slot * LPVMPC_EVENT_I32, run * LPVMPC_EVENT_I32 * 4);
        if (f64) D2H(f64 + j * LPVMPC_EVENT_F64, q->d.ev_f + slot * LPVMPC_EVENT_F64, run * LPVMPC_EVENT_F64 * 8);
        j += run;
    }
    RC_TRY(lpvmpc_event_planes(q->d, q->d.B).read(h, st, nullptr, out_i32));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (total) total[0] = (int64_t)tot;
    if (kept) kept[0] = (int32_t)k;
    return LPVMPC_OK;
}

// one tick on caller-supplied data; one-off device buffers, freed when the call returns
extern "C" int lpvmpc_event_step_batch(lpvmpc_handle *h, int32_t B, int32_t t, const int32_t *phase, const int32_t *lap, const double *lap_value,
                                       int32_t n_heats, const int32_t *heat, const double *heat_f64, const int32_t *heat_i32,
                                       const double *wall_f64, const int32_t *wall_i32, uint32_t kinds, double *carry_f64, int32_t *carry_i32,
                                       int64_t *total, int32_t max_events, int32_t *i32, double *f64, int32_t *n_events, int32_t *out_i32) {
    const char *who = "lpvmpc_event_step_batch";
    int rc;
    if (lpvmpc_batch_done(h, B, who, rc)) return rc;
    if (B < 0 || max_events < 0 || !phase || !lap || !lap_value || !carry_f64 || !carry_i32 || !total || !n_events || !out_i32 ||
        (max_events > 0 && (!i32 || !f64)))
        return fail(h, LPVMPC_E_ARG, "%s: B < 0, max_events < 0 or NULL argument", who);
    const bool heats = heat || heat_f64 || heat_i32, walls = wall_f64 || wall_i32;
    if (heats && (!heat || !heat_f64 || !heat_i32 || n_heats < 0))
        return fail(h, LPVMPC_E_ARG, "%s: the heats' side needs heat, heat_f64 and heat_i32 (all NULL: no heats) and n_heats >= 0", who);
    if (walls && (!wall_f64 || !wall_i32)) return fail(h, LPVMPC_E_ARG, "%s: the walls' side needs wall_f64 and wall_i32 (both NULL: no walls)", who);
    if (total[0] < 0) return fail(h, LPVMPC_E_ARG, "%s: total = %lld < 0", who, (long long)total[0]);
    RC_TRY(check_kinds(h, who, kinds));
    std::vector<int32_t> off, members;
    int largest = 0;
    if (heats) RC_TRY(lpvmpc_heat_members(h, who, B, n_heats, heat, off, members, largest));
    const size_t n = B, cap = max_events;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;
    lpvmpc::EventDev e{};
    lpvmpc::EventSrc s{};
    const Planes pl = lpvmpc_event_planes(e, n);
    HeatLists lists;
    int32_t *d_phase = nullptr, *d_lap = nullptr, *d_heat = nullptr, *d_hi = nullptr, *d_wi = nullptr;
    double *d_lapv = nullptr, *d_hf = nullptr, *d_wf = nullptr;
    DevTake take{mem};
    pl.alloc(take);
    take(d_phase, n * 4); take(d_lap, n * 4); take(d_lapv, n * 8);
    take(e.ev_i, cap * LPVMPC_EVENT_I32 * 4); take(e.ev_f, cap * LPVMPC_EVENT_F64 * 8); take(e.total, 8); take(e.n_events, 4);
    if (heats) { lists.alloc(take, off, members); take(d_heat, n * 4); take(d_hf, n * LPVMPC_HEAT_F64 * 8); take(d_hi, n * LPVMPC_HEAT_I32 * 4); }
    if (walls) { take(d_wf, n * LPVMPC_WALL_F64 * 8); take(d_wi, n * LPVMPC_WALL_I32 * 4); }
    RC_TRY(take.check(h, who, false));
    e.B = B; e.kinds = kinds; e.capacity = max_events;
    s.phase = d_phase; s.lap = d_lap; s.lap_value = d_lapv;
    if (heats) { s.heat_f = d_hf; s.heat_i = d_hi; s.heat_of = d_heat; s.off = lists.off; s.members = lists.members; s.n_heats = n_heats; }
    if (walls) { s.wall_f = d_wf; s.wall_i = d_wi; }
    const unsigned long long tot = (unsigned long long)total[0];
    hipStream_t st = h->stream;
    return lpvmpc_run_synced(h, st, [&]() -> int {                              // nothing in flight reads the buffers when they are freed
        H2D(d_phase, phase, n * 4); H2D(d_lap, lap, n * 4); H2D(d_lapv, lap_value, n * 8); H2D(e.total, &tot, 8);
        if (heats) {
            RC_TRY(lists.upload(h, st, off, members));
            H2D(d_heat, heat, n * 4); H2D(d_hf, heat_f64, n * LPVMPC_HEAT_F64 * 8); H2D(d_hi, heat_i32, n * LPVMPC_HEAT_I32 * 4);
        }
        if (walls) { H2D(d_wf, wall_f64, n * LPVMPC_WALL_F64 * 8); H2D(d_wi, wall_i32, n * LPVMPC_WALL_I32 * 4); }
        RC_TRY(pl.carry_in(h, st, carry_f64, carry_i32));
        if (max_events > 0) {                                                   // slots past the tick's count read -1 / NaN
            HIP_TRY(h, hipMemsetAsync(e.ev_i, 0xff, cap * LPVMPC_EVENT_I32 * 4, st));
            HIP_TRY(h, hipMemsetAsync(e.ev_f, 0xff, cap * LPVMPC_EVENT_F64 * 8, st));
        }
        HIP_TRY(h, lpvmpc::launch_event_step(e, s, t, st));
        D2H(total, e.total, 8); D2H(n_events, e.n_events, 4);
        if (max_events > 0) {
            D2H(i32, e.ev_i, cap * LPVMPC_EVENT_I32 * 4); D2H(f64, e.ev_f, cap * LPVMPC_EVENT_F64 * 8);
        }
        return pl.copy_out(h, st, carry_f64, carry_i32, nullptr, out_i32);
    });
}
