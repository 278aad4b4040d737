// interactions_api.hip -- C ABI of the interactions (include/lpvmpc.h, "Interactions"): attaching them to a race with heats, reading
// the outputs, and the stand-alone tick on caller-supplied data.  Kernel: interactions.hip.  The binding lives in the race next to the
// heats (race_api.hip owns the slot and launches the tick's kernel behind the disturbances'); it is built in a local and installed only
// when it is whole.
#include <cmath>
#include <new>
#include <vector>

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

extern "C" int lpvmpc_race_interactions(lpvmpc_handle *h, const lpvmpc_interaction_config *cfg) {
    const char *who = "lpvmpc_race_interactions";
    RaceAttach a;
    RC_TRY(a.begin(h, who));
    const RaceAttachView &v = a.v;
    hipStream_t st = a.st;
    if (!cfg) return lpvmpc_race_detach(h, RACE_INTERACTIONS);
    const HeatsBinding *heats = v.heats->get();
    if (!heats) return fail(h, LPVMPC_E_ARG, "%s: no heats are attached (lpvmpc_race_heats): the interactions act within a heat", who);
    if (!v.side->veh.d.p)
        return fail(h, LPVMPC_E_ARG, "%s: the race has no plant table (start it through lpvmpc_race_init_vehicles / lpvmpc_race_init_tyres): there is "
                    "no mass to exchange an impulse with and no drag word to scale", who);
    RC_TRY(check_config(h, who, cfg));
    RC_TRY(lpvmpc_race_detach_readers(h, RACE_INTERACTIONS));                   // the contact model reads the binding that is replaced
    HIP_TRY(h, hipStreamSynchronize(st));                                       // no tick in flight writes the table read below
    std::unique_ptr<InterBinding> q(new (std::nothrow) InterBinding());         // installed once it is complete
    if (!q) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    const size_t B = v.B;
    double *live = const_cast<double *>(v.side->veh.d.p);                       // [7][B]
    const InterBinding *old = v.inter->get();
    if (old) q->mu_base = old->mu_base;                                         // attached already: the live words may be scaled
    else {
        q->mu_base.resize(B);
        D2H(q->mu_base.data(), live + 6 * B, B * 8);
        HIP_TRY(h, hipStreamSynchronize(st));
    }
    lpvmpc::InterDev &e = q->d;
    const lpvmpc::HeatDev &hd = heats->d;
    const Planes pl = lpvmpc_interaction_planes(e, B);
    double *d_base = nullptr;
    DevTake take{q->mem};
    take(d_base, B * 8); pl.alloc(take);
    RC_TRY(take.check(h, who, true));
    e.B = v.B; e.n_heats = hd.n_heats; e.hl = hd.hl; e.hwc = hd.hwc; e.off = hd.off; e.members = hd.members;
    set_config(*cfg, e);
    e.plant = v.plant; e.nstep = v.nstep; e.m = live + 2 * B; e.mu_base = d_base; e.mu_live = live + 6 * B;
    q->block = heats->block; q->cfg = *cfg;
    std::vector<int32_t> heat_of, ci(B * LPVMPC_INTER_CARRY_I32, 0), i;
    std::vector<double> f;
    return lpvmpc_race_install(h, st, *v.inter, q, [&]() -> int {
        RC_TRY(lpvmpc_heat_of(h, st, hd.n_heats, hd.off, hd.members, B, heat_of));
        blank_outputs(B, heat_of.data(), q->mu_base.data(), f, i);
        for (size_t b = 0; b < B; ++b) ci[(size_t)LPVMPC_INTER_CARRY_FIRST_HIT_TICK * B + b] = -1;
        H2D(d_base, q->mu_base.data(), B * 8);
        RC_TRY(pl.blank_carry(h, st, ci.data()));
        RC_TRY(pl.blank_out(h, st, f, i));
        if (old) H2D(live + 6 * B, q->mu_base.data(), B * 8);                    // a vehicle the new binding never steps keeps the base word
        return LPVMPC_OK;
    });
}

static Planes read_planes(InterBinding &q) { return lpvmpc_interaction_planes(q.d, q.d.B); }

extern "C" int lpvmpc_race_interactions_read(lpvmpc_handle *h, double *f64, int32_t *i32) {
    return lpvmpc_race_read_planes(h, "lpvmpc_race_interactions_read", &RaceAttachView::inter,
                                   "no interactions are attached (lpvmpc_race_interactions)", read_planes, f64, i32);
}

// one tick on caller-supplied data; one-off device buffers, freed when the call returns
extern "C" int lpvmpc_interaction_step_batch(lpvmpc_handle *h, int32_t B, int32_t n_heats, const int32_t *heat, const lpvmpc_heats_config *heats_cfg,
                                             const lpvmpc_interaction_config *cfg, int32_t t, double *plant, const double *plant_params,
                                             const int32_t *nstep, double *carry_f64, int32_t *carry_i32, double *mu_live, double *f64, int32_t *i32) {
    const char *who = "lpvmpc_interaction_step_batch";
    int rc;
    if (lpvmpc_batch_done(h, B, who, rc)) return rc;
    if (B < 0 || n_heats < 0 || !heat || !cfg || !plant || !plant_params || !carry_f64 || !carry_i32 || !mu_live || !f64 || !i32)
        return fail(h, LPVMPC_E_ARG, "%s: B < 0, n_heats < 0 or NULL argument", who);
    RC_TRY(lpvmpc_heat_extents(h, who, heats_cfg));
    RC_TRY(check_config(h, who, cfg));
    std::vector<int32_t> off, members;
    int largest = 0;
    RC_TRY(lpvmpc_heat_members(h, who, B, n_heats, heat, off, members, largest));
    std::vector<double> tab;                                                    // [7][B], checked (m > 0, mu >= 0)
    RC_TRY(lpvmpc_plant_rows(h, B, plant_params, h->cfg, 0.0, who, tab));
    const size_t n = B;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;
    lpvmpc::InterDev e{};
    const Planes pl = lpvmpc_interaction_planes(e, n);
    HeatLists lists;
    double *d_m = nullptr, *d_base = nullptr;
    int32_t *d_nstep = nullptr;
    DevTake take{mem};
    lists.alloc(take, off, members); take(e.plant, n * 8 * 8); take(d_m, n * 8); take(d_base, n * 8);
    take(e.mu_live, n * 8);
    if (nstep) take(d_nstep, n * 4);
    pl.alloc(take);
    RC_TRY(take.check(h, who, false));
    e.B = B; e.n_heats = n_heats; e.hl = heats_cfg->half_length; e.hwc = heats_cfg->half_width_car;
    e.off = lists.off; e.members = lists.members; e.nstep = d_nstep; e.m = d_m; e.mu_base = d_base;
    set_config(*cfg, e);
    std::vector<double> f;
    std::vector<int32_t> i;
    blank_outputs(n, heat, tab.data() + 6 * n, f, i);
    hipStream_t st = h->stream;
    return lpvmpc_run_synced(h, st, [&]() -> int {                              // nothing in flight reads the buffers when they are freed
        RC_TRY(lists.upload(h, st, off, members));
        H2D(e.plant, plant, n * 8 * 8); H2D(d_m, tab.data() + 2 * n, n * 8); H2D(d_base, tab.data() + 6 * n, n * 8);
        H2D(e.mu_live, tab.data() + 6 * n, n * 8);
        if (nstep) H2D(d_nstep, nstep, n * 4);
        RC_TRY(pl.carry_in(h, st, carry_f64, carry_i32));
        RC_TRY(pl.blank_out(h, st, f, i));
        HIP_TRY(h, lpvmpc::launch_interaction_tick(e, largest <= 64 ? 64 : 256, t, st));
        D2H(plant, e.plant, n * 8 * 8); D2H(mu_live, e.mu_live, n * 8);
        return pl.copy_out(h, st, carry_f64, carry_i32, f64, i32);
    });
}
