// interactions_api.hip -- C ABI of the interactions (include/lpvmpc.h, "Interactions"): attaching them to a race with heats, reading
// the outputs, and the stand-alone tick on caller-supplied data.  Kernel: interactions.hip.  The binding lives in the race next to the
// heats (race_api.hip owns the slot and launches the tick's kernel behind the disturbances'); it is built in a local and installed only
// when it is whole.
#include <cmath>
#include <new>
#include <vector>

#include "contact_host.hpp"
#include "interactions_host.hpp"

namespace {

int check_config(lpvmpc_handle *h, const char *who, const lpvmpc_interaction_config *c) {
    const double w[5] = {c->draft_gain, c->wake_length, c->wake_half_width, c->restitution, c->push};
    for (double v : w)
        if (!std::isfinite(v)) return fail(h, LPVMPC_E_ARG, "%s: a word of the configuration is not finite", who);
    if (c->draft_gain < 0 || c->draft_gain > 1 || !(c->wake_length > 0) || !(c->wake_half_width > 0) || (c->contact != 0 && c->contact != 1) ||
        c->restitution < 0 || c->restitution > 1 || c->push < 0 || c->push > 1)
        return fail(h, LPVMPC_E_ARG, "%s: draft_gain = %g, wake_length = %g, wake_half_width = %g, contact = %d, restitution = %g, push = %g (draft_gain, "
                    "restitution, push in [0, 1]; wake_length, wake_half_width > 0; contact 0 / 1)", who, c->draft_gain, c->wake_length,
                    c->wake_half_width, c->contact, c->restitution, c->push);
    return LPVMPC_OK;
}

void set_config(const lpvmpc_interaction_config &c, lpvmpc::InterDev &d) {
    d.draft_gain = c.draft_gain; d.wake_length = c.wake_length; d.wake_half_width = c.wake_half_width; d.restitution = c.restitution;
    d.push = c.push; d.contact = c.contact;
}

// what a vehicle reads before its first tick: no heat NaN / -1 / 0, a member shelter 0, its base mu, no impulse, no leader, no hit
void blank_outputs(size_t B, const int32_t *heat_of, const double *mu, std::vector<double> &f, std::vector<int32_t> &i) {
    f.assign(B * LPVMPC_INTER_F64, std::nan(""));
    i.assign(B * LPVMPC_INTER_I32, 0);
    for (size_t b = 0; b < B; ++b) {
        i[(size_t)LPVMPC_INTER_LEADER * B + b] = -1; i[(size_t)LPVMPC_INTER_FIRST_HIT_TICK * B + b] = -1;
        if (heat_of[b] < 0) continue;
        for (int c = 0; c < LPVMPC_INTER_F64; ++c) f[(size_t)c * B + b] = 0.0;
        f[(size_t)LPVMPC_INTER_MU * B + b] = mu[b];
    }
}

}  // namespace

// the three above for contact_api.hip (interactions_host.hpp)
int lpvmpc_interaction_check_config(lpvmpc_handle *h, const char *who, const lpvmpc_interaction_config *c) { return check_config(h, who, c); }
void lpvmpc_interaction_set_config(const lpvmpc_interaction_config &c, lpvmpc::InterDev &d) { set_config(c, d); }
void lpvmpc_interaction_blank_outputs(size_t B, const int32_t *heat_of, const double *mu, std::vector<double> &f, std::vector<int32_t> &i) {
    blank_outputs(B, heat_of, mu, f, i);
}

extern "C" void lpvmpc_interaction_default_config(lpvmpc_interaction_config *c) {
    if (!c) return;
    // invented values of the right order for a 1:10 car (0.8 m long): nothing in the reference fixes them
    c->draft_gain = 0.3; c->wake_length = 3.0; c->wake_half_width = 0.3; c->contact = 1; c->reserved = 0; c->restitution = 0.2; c->push = 0.5;
}

int lpvmpc_race_interactions_detach(lpvmpc_handle *h) {
    RaceInterView v;
    if (!h || !lpvmpc_race_inter_view(h, v) || !v.slot->get()) return LPVMPC_OK;
    { const int rd = lpvmpc_race_contact_detach(h); if (rd) return rd; }        // the contact model reads this binding
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));                                       // no tick in flight reads the binding
    const InterBinding &q = **v.slot;
    H2D(q.d.mu_live, q.mu_base.data(), q.mu_base.size() * 8);                   // the base words back to the live table
    HIP_TRY(h, hipStreamSynchronize(st));
    v.slot->reset();
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_interactions(lpvmpc_handle *h, const lpvmpc_interaction_config *cfg) {
    const char *who = "lpvmpc_race_interactions";
    RaceInterView v;
    if (!h || !lpvmpc_race_inter_view(h, v)) return fail(h, LPVMPC_E_ARG, "%s: call lpvmpc_race_init first", who);
    if (!cfg) return lpvmpc_race_interactions_detach(h);
    if (!v.heats) return fail(h, LPVMPC_E_ARG, "%s: no heats are attached (lpvmpc_race_heats): the interactions act within a heat", who);
    if (!v.side->veh.d.p)
        return fail(h, LPVMPC_E_ARG, "%s: the race has no plant table (start it through lpvmpc_race_init_vehicles / lpvmpc_race_init_tyres): there is "
                    "no mass to exchange an impulse with and no drag word to scale", who);
    int rc = check_config(h, who, cfg); if (rc) return rc;
    rc = lpvmpc_race_contact_detach(h); if (rc) return rc;                      // the contact model reads the binding that is replaced
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));                                       // no tick in flight writes the table read below
    std::unique_ptr<InterBinding> q(new (std::nothrow) InterBinding());         // installed once it is complete
    if (!q) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    const size_t B = v.B;
    double *live = const_cast<double *>(v.side->veh.d.p);                       // [7][B]
    const InterBinding *old = v.slot->get();
    if (old) q->mu_base = old->mu_base;                                         // attached already: the live words may be scaled
    else {
        q->mu_base.resize(B);
        D2H(q->mu_base.data(), live + 6 * B, B * 8);
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    lpvmpc::InterDev &e = q->d;
    const lpvmpc::HeatDev &hd = v.heats->d;
    double *d_base = nullptr;
    hipError_t err = hipSuccess;
    size_t want = 0;
    auto take = [&](auto *&p, size_t n) { if (err == hipSuccess) { want = n; err = q->mem.alloc(p, n ? n : 8); } };
    take(d_base, B * 8); take(e.carry_f, B * LPVMPC_INTER_CARRY_F64 * 8); take(e.carry_i, B * LPVMPC_INTER_CARRY_I32 * 4);
    take(e.out_f, B * LPVMPC_INTER_F64 * 8); take(e.out_i, B * LPVMPC_INTER_I32 * 4);
    if (err != hipSuccess) return fail(h, LPVMPC_E_NOMEM, "%s: hipMalloc of %zu B failed: %s", who, want, hipGetErrorString(err));
    e.B = v.B; e.n_heats = hd.n_heats; e.hl = hd.hl; e.hwc = hd.hwc; e.off = hd.off; e.members = hd.members;
    set_config(*cfg, e);
    e.plant = v.plant; e.nstep = v.nstep; e.m = live + 2 * B; e.mu_base = d_base; e.mu_live = live + 6 * B;
    q->block = v.heats->block; q->cfg = *cfg;
    // the heat of each vehicle, from the heats' lists as they were uploaded
    std::vector<int32_t> off((size_t)hd.n_heats + 1), members, heat_of(B, -1), ci(B * LPVMPC_INTER_CARRY_I32, 0), i;
    std::vector<double> f;
    auto run = [&]() -> int {
        D2H(off.data(), hd.off, off.size() * 4);
        HIP_TRY(h, hipStreamSynchronize(st));
        members.resize((size_t)off[hd.n_heats]);
        if (!members.empty()) D2H(members.data(), hd.members, members.size() * 4);
        HIP_TRY(h, hipStreamSynchronize(st));
        for (int g = 0; g < hd.n_heats; ++g)
            for (int k = off[g]; k < off[g + 1]; ++k) heat_of[(size_t)members[k]] = g;
        blank_outputs(B, heat_of.data(), q->mu_base.data(), f, i);
        for (size_t b = 0; b < B; ++b) ci[(size_t)LPVMPC_INTER_CARRY_FIRST_HIT_TICK * B + b] = -1;
        H2D(d_base, q->mu_base.data(), B * 8);
        HIP_TRY(h, hipMemsetAsync(e.carry_f, 0, B * LPVMPC_INTER_CARRY_F64 * 8, st));
        H2D(e.carry_i, ci.data(), ci.size() * 4);
        H2D(e.out_f, f.data(), f.size() * 8);
        H2D(e.out_i, i.data(), i.size() * 4);
        if (old) H2D(live + 6 * B, q->mu_base.data(), B * 8);                    // a vehicle the new binding never steps keeps the base word
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    rc = run();
    if (rc) { (void)hipStreamSynchronize(st); return rc; }                      // the host vectors outlive the copies; nothing installed
    *v.slot = std::move(q);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_interactions_read(lpvmpc_handle *h, double *f64, int32_t *i32) {
    const char *who = "lpvmpc_race_interactions_read";
    RaceInterView v;
    if (!h || !lpvmpc_race_inter_view(h, v)) return fail(h, LPVMPC_E_ARG, "%s: call lpvmpc_race_init first", who);
    const InterBinding *q = v.slot->get();
    if (!q) return fail(h, LPVMPC_E_ARG, "%s: no interactions are attached (lpvmpc_race_interactions)", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t B = q->d.B;
    if (f64) D2H(f64, q->d.out_f, B * LPVMPC_INTER_F64 * 8);
    if (i32) D2H(i32, q->d.out_i, B * LPVMPC_INTER_I32 * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

// one tick on caller-supplied data; one-off device buffers, freed when the call returns
extern "C" int lpvmpc_interaction_step_batch(lpvmpc_handle *h, int32_t B, int32_t n_heats, const int32_t *heat, const lpvmpc_heats_config *heats_cfg,
                                             const lpvmpc_interaction_config *cfg, int32_t t, double *plant, const double *plant_params,
                                             const int32_t *nstep, double *carry_f64, int32_t *carry_i32, double *mu_live, double *f64, int32_t *i32) {
    const char *who = "lpvmpc_interaction_step_batch";
    if (h && B == 0) return LPVMPC_OK;
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h)) return fail(h, LPVMPC_E_ARG, "%s: this handle runs a fleet, cascade or race; use another handle for batch calls", who);
    if (B < 0 || n_heats < 0 || !heat || !cfg || !plant || !plant_params || !carry_f64 || !carry_i32 || !mu_live || !f64 || !i32)
        return fail(h, LPVMPC_E_ARG, "%s: B < 0, n_heats < 0 or NULL argument", who);
    int rc = lpvmpc_heat_extents(h, who, heats_cfg); if (rc) return rc;
    rc = check_config(h, who, cfg); if (rc) return rc;
    std::vector<int32_t> off, members;
    int largest = 0;
    rc = lpvmpc_heat_members(h, who, B, n_heats, heat, off, members, largest); if (rc) return rc;
    std::vector<double> tab;                                                    // [7][B], checked (m > 0, mu >= 0)
    rc = lpvmpc_plant_rows(h, B, plant_params, h->cfg, 0.0, who, tab); if (rc) return rc;
    const size_t n = B;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;
    lpvmpc::InterDev e{};
    double *d_m = nullptr, *d_base = nullptr;
    int32_t *d_off = nullptr, *d_members = nullptr, *d_nstep = nullptr;
    hipError_t err = hipSuccess;
    auto take = [&](auto *&p, size_t bytes) { if (err == hipSuccess) err = mem.alloc(p, bytes ? bytes : 8); };
    take(d_off, off.size() * 4); take(d_members, members.size() * 4); take(e.plant, n * 8 * 8); take(d_m, n * 8); take(d_base, n * 8);
    take(e.mu_live, n * 8);
    if (nstep) take(d_nstep, n * 4);
    take(e.carry_f, n * LPVMPC_INTER_CARRY_F64 * 8); take(e.carry_i, n * LPVMPC_INTER_CARRY_I32 * 4);
    take(e.out_f, n * LPVMPC_INTER_F64 * 8); take(e.out_i, n * LPVMPC_INTER_I32 * 4);
    if (err != hipSuccess) return fail(h, LPVMPC_E_NOMEM, "%s: hipMalloc failed: %s", who, hipGetErrorString(err));
    e.B = B; e.n_heats = n_heats; e.hl = heats_cfg->half_length; e.hwc = heats_cfg->half_width_car;
    e.off = d_off; e.members = d_members; e.nstep = d_nstep; e.m = d_m; e.mu_base = d_base;
    set_config(*cfg, e);
    std::vector<double> f;
    std::vector<int32_t> i;
    blank_outputs(n, heat, tab.data() + 6 * n, f, i);
    hipStream_t st = h->stream;
    auto run = [&]() -> int {
        H2D(d_off, off.data(), off.size() * 4);
        if (!members.empty()) H2D(d_members, members.data(), members.size() * 4);
        H2D(e.plant, plant, n * 8 * 8); H2D(d_m, tab.data() + 2 * n, n * 8); H2D(d_base, tab.data() + 6 * n, n * 8);
        H2D(e.mu_live, tab.data() + 6 * n, n * 8);
        if (nstep) H2D(d_nstep, nstep, n * 4);
        H2D(e.carry_f, carry_f64, n * LPVMPC_INTER_CARRY_F64 * 8); H2D(e.carry_i, carry_i32, n * LPVMPC_INTER_CARRY_I32 * 4);
        H2D(e.out_f, f.data(), f.size() * 8); H2D(e.out_i, i.data(), i.size() * 4);
        HIP_TRY(h, lpvmpc::launch_interaction_tick(e, largest <= 64 ? 64 : 256, t, st));
        D2H(plant, e.plant, n * 8 * 8); D2H(mu_live, e.mu_live, n * 8);
        D2H(carry_f64, e.carry_f, n * LPVMPC_INTER_CARRY_F64 * 8); D2H(carry_i32, e.carry_i, n * LPVMPC_INTER_CARRY_I32 * 4);
        D2H(f64, e.out_f, f.size() * 8); D2H(i32, e.out_i, i.size() * 4);
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);                                             // nothing in flight reads the buffers when they are freed
    return rc;
}
