// heats_api.hip -- C ABI of the heats (include/lpvmpc.h, "Heats"): attaching heats to a race, reading the standings, and the
// stand-alone tick on caller-supplied data.  Kernels: heats.hip.  The attachment lives in the race (race_api.hip owns the slot and
// launches the tick's kernel behind the recorder's); it is built in a local and installed only when it is whole.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "heats_host.hpp"

// member lists of the heats: off [n_heats + 1], members in ascending vehicle index within each heat (a counting sort keeps the order)
int lpvmpc_heat_members(lpvmpc_handle *h, const char *who, int B, int n_heats, const int32_t *heat, std::vector<int32_t> &off, std::vector<int32_t> &members,
                 int &largest) {
    off.assign((size_t)n_heats + 1, 0);
    for (int b = 0; b < B; ++b) {
        if (heat[b] < -1 || heat[b] >= n_heats)
            return fail(h, LPVMPC_E_ARG, "%s: heat[%d] = %d is outside [-1, %d)", who, b, heat[b], n_heats);
        if (heat[b] >= 0) off[(size_t)heat[b] + 1]++;
    }
    largest = 0;
    for (int g = 0; g < n_heats; ++g) {
        if (off[(size_t)g + 1] > LPVMPC_HEAT_MAX)
            return fail(h, LPVMPC_E_ARG, "%s: heat %d has %d members, at most %d", who, g, off[(size_t)g + 1], LPVMPC_HEAT_MAX);
        if (off[(size_t)g + 1] > largest) largest = off[(size_t)g + 1];
        off[(size_t)g + 1] += off[g];
    }
    members.assign((size_t)off[n_heats], 0);
    std::vector<int32_t> at(off.begin(), off.end() - 1);
    for (int b = 0; b < B; ++b) if (heat[b] >= 0) members[(size_t)at[heat[b]]++] = b;
    return LPVMPC_OK;
}

int lpvmpc_heat_extents(lpvmpc_handle *h, const char *who, const lpvmpc_heats_config *cfg) {
    if (!cfg) return fail(h, LPVMPC_E_ARG, "%s: the heats configuration is NULL", who);
    if (!(std::isfinite(cfg->half_length) && cfg->half_length > 0 && std::isfinite(cfg->half_width_car) && cfg->half_width_car > 0))
        return fail(h, LPVMPC_E_ARG, "%s: half_length = %g, half_width_car = %g must be finite and > 0", who, cfg->half_length, cfg->half_width_car);
    return LPVMPC_OK;
}

namespace {

// what a vehicle in no heat reads, and every vehicle before the first tick (a member's turns then reads its turns0)
void blank_standings(size_t B, const int32_t *heat, const int32_t *turns0, std::vector<double> &f, std::vector<int32_t> &i) {
    f.assign(B * LPVMPC_HEAT_F64, std::nan(""));
    i.assign(B * LPVMPC_HEAT_I32, 0);
    for (int c : {LPVMPC_HEAT_POSITION, LPVMPC_HEAT_AHEAD, LPVMPC_HEAT_NEAREST, LPVMPC_HEAT_FIRST_CONTACT_TICK, LPVMPC_HEAT_CLASS})
        for (size_t b = 0; b < B; ++b) i[(size_t)c * B + b] = -1;
    if (turns0) for (size_t b = 0; b < B; ++b) if (heat[b] >= 0) i[(size_t)LPVMPC_HEAT_TURNS * B + b] = turns0[b];
}

}  // namespace

extern "C" void lpvmpc_heats_default_config(lpvmpc_heats_config *c) {
    if (!c) return;
    c->half_length = 0.4; c->half_width_car = 0.2;      // the reference's drawn car (plotCarTrajectory.py:115,161-166)
}

extern "C" int lpvmpc_race_heats(lpvmpc_handle *h, const lpvmpc_heats_config *cfg, const int32_t *heat, const int32_t *turns0) {
    const char *who = "lpvmpc_race_heats";
    RaceAttach a;
    RC_TRY(a.begin(h, who));
    const RaceAttachView &v = a.v;
    hipStream_t st = a.st;
    std::vector<int32_t> off, members;
    int largest = 0, n_heats = 0;
    if (heat) {                                                                 // every check before the old attachment goes
        RC_TRY(lpvmpc_heat_extents(h, who, cfg));
        // indices need not be dense: the heats in use, in ascending order, take the workgroups of the launch (an empty heat takes none)
        std::vector<int32_t> ids;
        for (int b = 0; b < v.B; ++b) {
            if (heat[b] < -1) return fail(h, LPVMPC_E_ARG, "%s: heat[%d] = %d (-1: no heat)", who, b, heat[b]);
            if (heat[b] >= 0) ids.push_back(heat[b]);
        }
        std::sort(ids.begin(), ids.end());
        for (size_t k = 0, run = 0; k < ids.size(); ++k) {                      // the sizes, while the caller's indices are at hand
            run = k > 0 && ids[k] == ids[k - 1] ? run + 1 : 1;
            if (run > LPVMPC_HEAT_MAX) return fail(h, LPVMPC_E_ARG, "%s: heat %d has more than %d members", who, ids[k], LPVMPC_HEAT_MAX);
        }
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        n_heats = (int)ids.size();
        std::vector<int32_t> dense(v.B, -1);
        for (int b = 0; b < v.B; ++b)
            if (heat[b] >= 0) dense[b] = (int32_t)(std::lower_bound(ids.begin(), ids.end(), heat[b]) - ids.begin());
        RC_TRY(lpvmpc_heat_members(h, who, v.B, n_heats, dense.data(), off, members, largest));
        if (h->trk.tab)
            for (int g = 0; g < n_heats; ++g)
                for (int k = off[g] + 1; k < off[g + 1]; ++k)
                    if (h->trk_of[members[k]] != h->trk_of[members[off[g]]])
                        return fail(h, LPVMPC_E_ARG, "%s: heat %d: vehicle %d is on track %d, vehicle %d on track %d: a heat shares one track", who, ids[g],
                                    members[k], h->trk_of[members[k]], members[off[g]], h->trk_of[members[off[g]]]);
    }
    RC_TRY(lpvmpc_race_detach(h, RACE_HEATS));                                  // the old attachment goes first, and with it what reads it
    if (!heat) return LPVMPC_OK;
    std::unique_ptr<HeatsBinding> q(new (std::nothrow) HeatsBinding());         // installed once it is complete
    if (!q) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    lpvmpc::HeatDev &e = q->d;
    const size_t B = v.B, K = (size_t)v.laps + 2;
    const Planes pl = lpvmpc_heat_planes(e, B);
    HeatLists lists;
    DevTake take{q->mem};
    lists.alloc(take, off, members); pl.alloc(take);
    take(e.line_tick, B * K * 4); take(e.line_pos, B * K * 4);
    RC_TRY(take.check(h, who, true));
    e.B = v.B; e.n_heats = n_heats; e.K = (int)K; e.hl = cfg->half_length; e.hwc = cfg->half_width_car;
    e.off = lists.off; e.members = lists.members; e.plant = v.plant; e.hw = v.hw; e.slack = v.slack; e.phase = v.phase;
    q->block = largest <= 64 ? 64 : 256;
    std::vector<double> f;
    std::vector<int32_t> i;
    blank_standings(B, heat, turns0, f, i);
    return lpvmpc_race_install(h, st, *v.heats, q, [&]() -> int {
        RC_TRY(lists.upload(h, st, off, members));
        RC_TRY(pl.blank_carry(h, st, nullptr));
        if (turns0) H2D(e.carry_i + (size_t)LPVMPC_HEAT_CARRY_TURNS * B, turns0, B * 4);
        HIP_TRY(h, hipMemcpyAsync(e.carry_i + (size_t)LPVMPC_HEAT_CARRY_PHASE * B, v.phase, B * 4, hipMemcpyDeviceToDevice, st));
        RC_TRY(pl.blank_out(h, st, f, i));
        HIP_TRY(h, hipMemsetAsync(e.line_tick, 0xff, B * K * 4, st));
        HIP_TRY(h, hipMemsetAsync(e.line_pos, 0xff, B * K * 4, st));
        return LPVMPC_OK;
    }, v.heats_serial);
}

static Planes standings_planes(HeatsBinding &q) { return lpvmpc_heat_planes(q.d, q.d.B); }

extern "C" int lpvmpc_race_standings(lpvmpc_handle *h, double *f64, int32_t *i32, int32_t *line_tick, int32_t *line_pos) {
    return lpvmpc_race_read_planes(h, "lpvmpc_race_standings", &RaceAttachView::heats, "no heats are attached (lpvmpc_race_heats)", standings_planes,
                                   f64, i32, [&](HeatsBinding &q, hipStream_t st) -> int {
        const size_t B = q.d.B, K = q.d.K;
        if (line_tick) D2H(line_tick, q.d.line_tick, B * K * 4);
        if (line_pos) D2H(line_pos, q.d.line_pos, B * K * 4);
        return LPVMPC_OK;
    });
}

// one tick on caller-supplied data; one-off device buffers, freed when the call returns
extern "C" int lpvmpc_heat_step_batch(lpvmpc_handle *h, int32_t B, int32_t n_heats, const int32_t *heat, const double *L, const lpvmpc_heats_config *cfg,
                                      int32_t t, const double *pose, const double *s, const int32_t *inside, const int32_t *phase, double *carry_f64,
                                      int32_t *carry_i32, double *f64, int32_t *i32) {
    const char *who = "lpvmpc_heat_step_batch";
    int rc;
    if (lpvmpc_batch_done(h, B, who, rc)) return rc;
    if (B < 0 || n_heats < 0 || !heat || !L || !pose || !s || !inside || !phase || !carry_f64 || !carry_i32 || !f64 || !i32)
        return fail(h, LPVMPC_E_ARG, "%s: B < 0, n_heats < 0 or NULL argument", who);
    RC_TRY(lpvmpc_heat_extents(h, who, cfg));
    std::vector<int32_t> off, members;
    int largest = 0;
    RC_TRY(lpvmpc_heat_members(h, who, B, n_heats, heat, off, members, largest));
    const size_t n = B;
    for (size_t b = 0; b < n; ++b)
        if (heat[b] >= 0 && !(std::isfinite(L[b]) && L[b] > 0)) return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: L = %g must be finite and > 0", who, b, L[b]);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;
    lpvmpc::HeatDev e{};
    const Planes pl = lpvmpc_heat_planes(e, n);
    HeatLists lists;
    double *d_pose = nullptr, *d_s = nullptr, *d_L = nullptr;
    int32_t *d_inside = nullptr, *d_phase = nullptr;
    DevTake take{mem};
    lists.alloc(take, off, members); take(d_pose, n * 3 * 8); take(d_s, n * 8); take(d_L, n * 8);
    take(d_inside, n * 4); take(d_phase, n * 4);
    pl.alloc(take);
    RC_TRY(take.check(h, who, false));
    e.B = B; e.n_heats = n_heats; e.K = 0; e.hl = cfg->half_length; e.hwc = cfg->half_width_car;
    e.off = lists.off; e.members = lists.members; e.pose = d_pose; e.s = d_s; e.L = d_L; e.inside = d_inside; e.phase = d_phase;
    std::vector<double> f;
    std::vector<int32_t> i;
    blank_standings(n, heat, nullptr, f, i);
    hipStream_t st = h->stream;
    return lpvmpc_run_synced(h, st, [&]() -> int {                              // nothing in flight reads the buffers when they are freed
        RC_TRY(lists.upload(h, st, off, members));
        H2D(d_pose, pose, n * 3 * 8); H2D(d_s, s, n * 8); H2D(d_L, L, n * 8); H2D(d_inside, inside, n * 4); H2D(d_phase, phase, n * 4);
        RC_TRY(pl.carry_in(h, st, carry_f64, carry_i32));
        RC_TRY(pl.blank_out(h, st, f, i));
        HIP_TRY(h, lpvmpc::launch_heat_step(e, largest <= 64 ? 64 : 256, t, st));
        return pl.copy_out(h, st, carry_f64, carry_i32, f64, i32);
    });
}
