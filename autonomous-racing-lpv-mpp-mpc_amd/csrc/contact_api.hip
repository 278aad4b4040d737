// contact_api.hip -- C ABI of the contact model (include/lpvmpc.h, "Contact model"): attaching it on top of a race's interactions,
// reading its planes, and the stand-alone tick on caller-supplied data.  Kernel: contact.hip.  The binding lives in the race next to
// the interactions' (race_api.hip owns the slot and launches this kernel in place of theirs); it is built in a local and installed
// only when it is whole.
#include <cmath>
#include <new>
#include <vector>

#include "contact_host.hpp"

namespace {

int check_config(lpvmpc_handle *h, const char *who, const lpvmpc_contact_config *c) {
    if (!std::isfinite(c->friction)) return fail(h, LPVMPC_E_ARG, "%s: friction is not finite", who);
    if (c->friction < 0 || (c->yaw_response != 0 && c->yaw_response != 1) || c->reserved != 0)
        return fail(h, LPVMPC_E_ARG, "%s: friction = %g, yaw_response = %d, reserved = %d (friction >= 0; yaw_response 0 / 1; reserved 0)", who,
                    c->friction, c->yaw_response, c->reserved);
    return LPVMPC_OK;
}

// what a vehicle reads before its first tick: no heat NaN / 0, a member zeros
void blank_outputs(size_t B, const int32_t *heat_of, std::vector<double> &f, std::vector<int32_t> &i) {
    f.assign(B * LPVMPC_CONTACT_F64, std::nan(""));
    i.assign(B * LPVMPC_CONTACT_I32, 0);
    for (size_t b = 0; b < B; ++b) {
        if (heat_of[b] < 0) continue;
        for (int c = 0; c < LPVMPC_CONTACT_F64; ++c) f[(size_t)c * B + b] = 0.0;
    }
}

}  // namespace

extern "C" void lpvmpc_contact_default_config(lpvmpc_contact_config *c) {
    if (!c) return;
    c->friction = 0.3; c->yaw_response = 1; c->reserved = 0;                    // the walls' values
}

extern "C" int lpvmpc_race_contact(lpvmpc_handle *h, const lpvmpc_contact_config *cfg) {
    const char *who = "lpvmpc_race_contact";
    RaceAttach a;
    RC_TRY(a.begin(h, who));
    const RaceAttachView &v = a.v;
    hipStream_t st = a.st;
    if (!cfg) return lpvmpc_race_detach(h, RACE_CONTACT);
    const InterBinding *inter = v.inter->get();
    const HeatsBinding *heats = v.heats->get();
    if (!inter || !heats)
        return fail(h, LPVMPC_E_ARG, "%s: no interactions are attached (lpvmpc_race_interactions): the contact model is a form of their contact", who);
    if (!inter->cfg.contact) return fail(h, LPVMPC_E_ARG, "%s: the attached interactions have contact = 0: there is no contact to give a form to", who);
    RC_TRY(check_config(h, who, cfg));
    HIP_TRY(h, hipStreamSynchronize(st));
    std::unique_ptr<ContactBinding> q(new (std::nothrow) ContactBinding());     // installed once it is complete
    if (!q) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    const size_t B = v.B;
    lpvmpc::ContactDev &e = q->d;
    const Planes pl = lpvmpc_contact_planes(e, B);
    DevTake take{q->mem};
    pl.alloc(take);
    RC_TRY(take.check(h, who, true));
    e.i = inter->d;
    e.friction = cfg->friction; e.yaw_response = cfg->yaw_response;
    e.Iz = v.side->veh.d.p + 3 * B;                                             // row 3 of the live plant table [7][B]
    q->block = inter->block; q->cfg = *cfg;
    const lpvmpc::HeatDev &hd = heats->d;
    std::vector<int32_t> heat_of, i;
    std::vector<double> f;
    return lpvmpc_race_install(h, st, *v.contact, q, [&]() -> int {
        RC_TRY(lpvmpc_heat_of(h, st, hd.n_heats, hd.off, hd.members, B, heat_of));
        blank_outputs(B, heat_of.data(), f, i);
        RC_TRY(pl.blank_carry(h, st, nullptr));
        return pl.blank_out(h, st, f, i);
    });
}

static Planes read_planes(ContactBinding &q) { return lpvmpc_contact_planes(q.d, q.d.i.B); }

extern "C" int lpvmpc_race_contact_read(lpvmpc_handle *h, double *f64, int32_t *i32) {
    return lpvmpc_race_read_planes(h, "lpvmpc_race_contact_read", &RaceAttachView::contact, "no contact model is attached (lpvmpc_race_contact)",
                                   read_planes, f64, i32);
}

// one tick on caller-supplied data; one-off device buffers, freed when the call returns
extern "C" int lpvmpc_contact_step_batch(lpvmpc_handle *h, int32_t B, int32_t n_heats, const int32_t *heat, const lpvmpc_heats_config *heats_cfg,
                                         const lpvmpc_interaction_config *cfg, const lpvmpc_contact_config *contact_cfg, int32_t t, double *plant,
                                         const double *plant_params, const int32_t *nstep, double *carry_f64, int32_t *carry_i32,
                                         double *ccarry_f64, int32_t *ccarry_i32, double *mu_live, double *f64, int32_t *i32, double *cf64,
                                         int32_t *ci32) {
    const char *who = "lpvmpc_contact_step_batch";
    int rc;
    if (lpvmpc_batch_done(h, B, who, rc)) return rc;
    if (B < 0 || n_heats < 0 || !heat || !cfg || !contact_cfg || !plant || !plant_params || !carry_f64 || !carry_i32 || !ccarry_f64 || !ccarry_i32 ||
        !mu_live || !f64 || !i32 || !cf64 || !ci32)
        return fail(h, LPVMPC_E_ARG, "%s: B < 0, n_heats < 0 or NULL argument", who);
    RC_TRY(lpvmpc_heat_extents(h, who, heats_cfg));
    RC_TRY(lpvmpc_interaction_check_config(h, who, cfg));
    if (!cfg->contact) return fail(h, LPVMPC_E_ARG, "%s: the interactions' configuration has contact = 0: there is no contact to give a form to", who);
    RC_TRY(check_config(h, who, contact_cfg));
    std::vector<int32_t> off, members;
    int largest = 0;
    RC_TRY(lpvmpc_heat_members(h, who, B, n_heats, heat, off, members, largest));
    std::vector<double> tab;                                                    // [7][B], checked (m > 0, Iz > 0, mu >= 0)
    RC_TRY(lpvmpc_plant_rows(h, B, plant_params, h->cfg, 0.0, who, tab));
    const size_t n = B;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;
    lpvmpc::ContactDev d{};
    lpvmpc::InterDev &e = d.i;
    const Planes pl = lpvmpc_interaction_planes(e, n), kpl = lpvmpc_contact_planes(d, n);
    HeatLists lists;
    double *d_m = nullptr, *d_base = nullptr, *d_iz = nullptr;
    int32_t *d_nstep = nullptr;
    DevTake take{mem};
    lists.alloc(take, off, members); take(e.plant, n * 8 * 8); take(d_m, n * 8); take(d_base, n * 8);
    take(d_iz, n * 8); take(e.mu_live, n * 8);
    if (nstep) take(d_nstep, n * 4);
    pl.alloc(take); kpl.alloc(take);
    RC_TRY(take.check(h, who, false));
    e.B = B; e.n_heats = n_heats; e.hl = heats_cfg->half_length; e.hwc = heats_cfg->half_width_car;
    e.off = lists.off; e.members = lists.members; e.nstep = d_nstep; e.m = d_m; e.mu_base = d_base;
    lpvmpc_interaction_set_config(*cfg, e);
    d.friction = contact_cfg->friction; d.yaw_response = contact_cfg->yaw_response; d.Iz = d_iz;
    std::vector<double> f, kf;
    std::vector<int32_t> i, ki;
    lpvmpc_interaction_blank_outputs(n, heat, tab.data() + 6 * n, f, i);
    blank_outputs(n, heat, kf, ki);
    hipStream_t st = h->stream;
    return lpvmpc_run_synced(h, st, [&]() -> int {                              // nothing in flight reads the buffers when they are freed
        RC_TRY(lists.upload(h, st, off, members));
        H2D(e.plant, plant, n * 8 * 8); H2D(d_m, tab.data() + 2 * n, n * 8); H2D(d_iz, tab.data() + 3 * n, n * 8);
        H2D(d_base, tab.data() + 6 * n, n * 8); H2D(e.mu_live, tab.data() + 6 * n, n * 8);
        if (nstep) H2D(d_nstep, nstep, n * 4);
        RC_TRY(pl.carry_in(h, st, carry_f64, carry_i32));
        RC_TRY(kpl.carry_in(h, st, ccarry_f64, ccarry_i32));
        RC_TRY(pl.blank_out(h, st, f, i));
        RC_TRY(kpl.blank_out(h, st, kf, ki));
        HIP_TRY(h, lpvmpc::launch_contact_tick(d, largest <= 64 ? 64 : 256, t, st));
        D2H(plant, e.plant, n * 8 * 8); D2H(mu_live, e.mu_live, n * 8);
        RC_TRY(pl.copy_out(h, st, carry_f64, carry_i32, f64, i32));
        return kpl.copy_out(h, st, ccarry_f64, ccarry_i32, cf64, ci32);
    });
}
