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
    RaceHeatsView v;
    if (!h || !lpvmpc_race_heats_view(h, v)) return fail(h, LPVMPC_E_ARG, "%s: call lpvmpc_race_init first", who);
    std::vector<int32_t> off, members;
    int largest = 0, n_heats = 0;
    if (heat) {                                                                 // every check before the old attachment goes
        int rc = lpvmpc_heat_extents(h, who, cfg); if (rc) return rc;
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
        rc = lpvmpc_heat_members(h, who, v.B, n_heats, dense.data(), off, members, largest); if (rc) return rc;
        if (h->trk.tab)
            for (int g = 0; g < n_heats; ++g)
                for (int k = off[g] + 1; k < off[g + 1]; ++k)
                    if (h->trk_of[members[k]] != h->trk_of[members[off[g]]])
                        return fail(h, LPVMPC_E_ARG, "%s: heat %d: vehicle %d is on track %d, vehicle %d on track %d: a heat shares one track", who, ids[g],
                                    members[k], h->trk_of[members[k]], members[off[g]], h->trk_of[members[off[g]]]);
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));                                       // no tick in flight reads the old attachment
    { const int rd = lpvmpc_race_interactions_detach(h); if (rd) return rd; }   // the interactions read this attachment's lists and extents
    v.slot->reset();
    if (!heat) return LPVMPC_OK;
    std::unique_ptr<HeatsBinding> q(new (std::nothrow) HeatsBinding());         // installed once it is complete
    if (!q) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    lpvmpc::HeatDev &e = q->d;
    const size_t B = v.B, K = (size_t)v.laps + 2;
    int32_t *d_off = nullptr, *d_members = nullptr;
    hipError_t err = hipSuccess;
    size_t want = 0;
    auto take = [&](auto *&p, size_t n) { if (err == hipSuccess) { want = n; err = q->mem.alloc(p, n ? n : 8); } };
    take(d_off, off.size() * 4); take(d_members, members.size() * 4);
    take(e.carry_f, B * LPVMPC_HEAT_CARRY_F64 * 8); take(e.carry_i, B * LPVMPC_HEAT_CARRY_I32 * 4);
    take(e.out_f, B * LPVMPC_HEAT_F64 * 8); take(e.out_i, B * LPVMPC_HEAT_I32 * 4);
    take(e.line_tick, B * K * 4); take(e.line_pos, B * K * 4);
    if (err != hipSuccess) return fail(h, LPVMPC_E_NOMEM, "%s: hipMalloc of %zu B failed: %s", who, want, hipGetErrorString(err));
    e.B = v.B; e.n_heats = n_heats; e.K = (int)K; e.hl = cfg->half_length; e.hwc = cfg->half_width_car;
    e.off = d_off; e.members = d_members; e.plant = v.plant; e.hw = v.hw; e.slack = v.slack; e.phase = v.phase;
    q->block = largest <= 64 ? 64 : 256;
    std::vector<double> f;
    std::vector<int32_t> i;
    blank_standings(B, heat, turns0, f, i);
    auto run = [&]() -> int {
        H2D(d_off, off.data(), off.size() * 4);
        if (!members.empty()) H2D(d_members, members.data(), members.size() * 4);
        HIP_TRY(h, hipMemsetAsync(e.carry_f, 0, B * LPVMPC_HEAT_CARRY_F64 * 8, st));
        HIP_TRY(h, hipMemsetAsync(e.carry_i, 0, B * LPVMPC_HEAT_CARRY_I32 * 4, st));
        if (turns0) H2D(e.carry_i + (size_t)LPVMPC_HEAT_CARRY_TURNS * B, turns0, B * 4);
        HIP_TRY(h, hipMemcpyAsync(e.carry_i + (size_t)LPVMPC_HEAT_CARRY_PHASE * B, v.phase, B * 4, hipMemcpyDeviceToDevice, st));
        H2D(e.out_f, f.data(), f.size() * 8);
        H2D(e.out_i, i.data(), i.size() * 4);
        HIP_TRY(h, hipMemsetAsync(e.line_tick, 0xff, B * K * 4, st));
        HIP_TRY(h, hipMemsetAsync(e.line_pos, 0xff, B * K * 4, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    const int rc = run();
    if (rc) { (void)hipStreamSynchronize(st); return rc; }                      // the host vectors outlive the copies; nothing installed
    *v.slot = std::move(q);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_standings(lpvmpc_handle *h, double *f64, int32_t *i32, int32_t *line_tick, int32_t *line_pos) {
    const char *who = "lpvmpc_race_standings";
    RaceHeatsView v;
    if (!h || !lpvmpc_race_heats_view(h, v)) return fail(h, LPVMPC_E_ARG, "%s: call lpvmpc_race_init first", who);
    const HeatsBinding *q = v.slot->get();
    if (!q) return fail(h, LPVMPC_E_ARG, "%s: no heats are attached (lpvmpc_race_heats)", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t B = q->d.B, K = q->d.K;
    if (f64) D2H(f64, q->d.out_f, B * LPVMPC_HEAT_F64 * 8);
    if (i32) D2H(i32, q->d.out_i, B * LPVMPC_HEAT_I32 * 4);
    if (line_tick) D2H(line_tick, q->d.line_tick, B * K * 4);
    if (line_pos) D2H(line_pos, q->d.line_pos, B * K * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

// one tick on caller-supplied data; one-off device buffers, freed when the call returns
extern "C" int lpvmpc_heat_step_batch(lpvmpc_handle *h, int32_t B, int32_t n_heats, const int32_t *heat, const double *L, const lpvmpc_heats_config *cfg,
                                      int32_t t, const double *pose, const double *s, const int32_t *inside, const int32_t *phase, double *carry_f64,
                                      int32_t *carry_i32, double *f64, int32_t *i32) {
    const char *who = "lpvmpc_heat_step_batch";
    if (h && B == 0) return LPVMPC_OK;
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h)) return fail(h, LPVMPC_E_ARG, "%s: this handle runs a fleet, cascade or race; use another handle for batch calls", who);
    if (B < 0 || n_heats < 0 || !heat || !L || !pose || !s || !inside || !phase || !carry_f64 || !carry_i32 || !f64 || !i32)
        return fail(h, LPVMPC_E_ARG, "%s: B < 0, n_heats < 0 or NULL argument", who);
    int rc = lpvmpc_heat_extents(h, who, cfg); if (rc) return rc;
    std::vector<int32_t> off, members;
    int largest = 0;
    rc = lpvmpc_heat_members(h, who, B, n_heats, heat, off, members, largest); if (rc) return rc;
    const size_t n = B;
    for (size_t b = 0; b < n; ++b)
        if (heat[b] >= 0 && !(std::isfinite(L[b]) && L[b] > 0)) return fail(h, LPVMPC_E_ARG, "%s: vehicle %zu: L = %g must be finite and > 0", who, b, L[b]);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;
    lpvmpc::HeatDev e{};
    double *d_pose = nullptr, *d_s = nullptr, *d_L = nullptr;
    int32_t *d_off = nullptr, *d_members = nullptr, *d_inside = nullptr, *d_phase = nullptr;
    hipError_t err = hipSuccess;
    auto take = [&](auto *&p, size_t bytes) { if (err == hipSuccess) err = mem.alloc(p, bytes ? bytes : 8); };
    take(d_off, off.size() * 4); take(d_members, members.size() * 4); take(d_pose, n * 3 * 8); take(d_s, n * 8); take(d_L, n * 8);
    take(d_inside, n * 4); take(d_phase, n * 4);
    take(e.carry_f, n * LPVMPC_HEAT_CARRY_F64 * 8); take(e.carry_i, n * LPVMPC_HEAT_CARRY_I32 * 4);
    take(e.out_f, n * LPVMPC_HEAT_F64 * 8); take(e.out_i, n * LPVMPC_HEAT_I32 * 4);
    if (err != hipSuccess) return fail(h, LPVMPC_E_NOMEM, "%s: hipMalloc failed: %s", who, hipGetErrorString(err));
    e.B = B; e.n_heats = n_heats; e.K = 0; e.hl = cfg->half_length; e.hwc = cfg->half_width_car;
    e.off = d_off; e.members = d_members; e.pose = d_pose; e.s = d_s; e.L = d_L; e.inside = d_inside; e.phase = d_phase;
    std::vector<double> f;
    std::vector<int32_t> i;
    blank_standings(n, heat, nullptr, f, i);
    hipStream_t st = h->stream;
    auto run = [&]() -> int {
        H2D(d_off, off.data(), off.size() * 4);
        if (!members.empty()) H2D(d_members, members.data(), members.size() * 4);
        H2D(d_pose, pose, n * 3 * 8); H2D(d_s, s, n * 8); H2D(d_L, L, n * 8); H2D(d_inside, inside, n * 4); H2D(d_phase, phase, n * 4);
        H2D(e.carry_f, carry_f64, n * LPVMPC_HEAT_CARRY_F64 * 8); H2D(e.carry_i, carry_i32, n * LPVMPC_HEAT_CARRY_I32 * 4);
        H2D(e.out_f, f.data(), f.size() * 8); H2D(e.out_i, i.data(), i.size() * 4);
        HIP_TRY(h, lpvmpc::launch_heat_step(e, largest <= 64 ? 64 : 256, t, st));
        D2H(carry_f64, e.carry_f, n * LPVMPC_HEAT_CARRY_F64 * 8); D2H(carry_i32, e.carry_i, n * LPVMPC_HEAT_CARRY_I32 * 4);
        D2H(f64, e.out_f, f.size() * 8); D2H(i32, e.out_i, i.size() * 4);
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);                                             // nothing in flight reads the buffers when they are freed
    return rc;
}
