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

int lpvmpc_race_contact_detach(lpvmpc_handle *h) {
    RaceContactView v;
    if (!h || !lpvmpc_race_contact_view(h, v) || !v.slot->get()) return LPVMPC_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                                // no tick in flight reads the binding
    v.slot->reset();
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_contact(lpvmpc_handle *h, const lpvmpc_contact_config *cfg) {
    const char *who = "lpvmpc_race_contact";
    RaceContactView v;
    if (!h || !lpvmpc_race_contact_view(h, v)) return fail(h, LPVMPC_E_ARG, "%s: call lpvmpc_race_init first", who);
    if (!cfg) return lpvmpc_race_contact_detach(h);
    if (!v.inter || !v.heats)
        return fail(h, LPVMPC_E_ARG, "%s: no interactions are attached (lpvmpc_race_interactions): the contact model is a form of their contact", who);
    if (!v.inter->cfg.contact) return fail(h, LPVMPC_E_ARG, "%s: the attached interactions have contact = 0: there is no contact to give a form to", who);
    int rc = check_config(h, who, cfg); if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    HIP_TRY(h, hipStreamSynchronize(st));
    std::unique_ptr<ContactBinding> q(new (std::nothrow) ContactBinding());     // installed once it is complete
    if (!q) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    const size_t B = v.B;
    lpvmpc::ContactDev &e = q->d;
    hipError_t err = hipSuccess;
    size_t want = 0;
    auto take = [&](auto *&p, size_t n) { if (err == hipSuccess) { want = n; err = q->mem.alloc(p, n ? n : 8); } };
    take(e.carry_f, B * LPVMPC_CONTACT_CARRY_F64 * 8); take(e.carry_i, B * LPVMPC_CONTACT_CARRY_I32 * 4);
    take(e.out_f, B * LPVMPC_CONTACT_F64 * 8); take(e.out_i, B * LPVMPC_CONTACT_I32 * 4);
    if (err != hipSuccess) return fail(h, LPVMPC_E_NOMEM, "%s: hipMalloc of %zu B failed: %s", who, want, hipGetErrorString(err));
    e.i = v.inter->d;
    e.friction = cfg->friction; e.yaw_response = cfg->yaw_response;
    e.Iz = v.side->veh.d.p + 3 * B;                                             // row 3 of the live plant table [7][B]
    q->block = v.inter->block; q->cfg = *cfg;
    // the heat of each vehicle, from the heats' lists as they were uploaded
    const lpvmpc::HeatDev &hd = v.heats->d;
    std::vector<int32_t> off((size_t)hd.n_heats + 1), members, heat_of(B, -1), i;
    std::vector<double> f;
    auto run = [&]() -> int {
        D2H(off.data(), hd.off, off.size() * 4);
        HIP_TRY(h, hipStreamSynchronize(st));
        members.resize((size_t)off[hd.n_heats]);
        if (!members.empty()) D2H(members.data(), hd.members, members.size() * 4);
        HIP_TRY(h, hipStreamSynchronize(st));
        for (int g = 0; g < hd.n_heats; ++g)
            for (int k = off[g]; k < off[g + 1]; ++k) heat_of[(size_t)members[k]] = g;
        blank_outputs(B, heat_of.data(), f, i);
        HIP_TRY(h, hipMemsetAsync(e.carry_f, 0, B * LPVMPC_CONTACT_CARRY_F64 * 8, st));
        HIP_TRY(h, hipMemsetAsync(e.carry_i, 0, B * LPVMPC_CONTACT_CARRY_I32 * 4, st));
        H2D(e.out_f, f.data(), f.size() * 8);
        H2D(e.out_i, i.data(), i.size() * 4);
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    rc = run();
    if (rc) { (void)hipStreamSynchronize(st); return rc; }                      // the host vectors outlive the copies; nothing installed
    *v.slot = std::move(q);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_race_contact_read(lpvmpc_handle *h, double *f64, int32_t *i32) {
    const char *who = "lpvmpc_race_contact_read";
    RaceContactView v;
    if (!h || !lpvmpc_race_contact_view(h, v)) return fail(h, LPVMPC_E_ARG, "%s: call lpvmpc_race_init first", who);
    const ContactBinding *q = v.slot->get();
    if (!q) return fail(h, LPVMPC_E_ARG, "%s: no contact model is attached (lpvmpc_race_contact)", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t B = q->d.i.B;
    if (f64) D2H(f64, q->d.out_f, B * LPVMPC_CONTACT_F64 * 8);
    if (i32) D2H(i32, q->d.out_i, B * LPVMPC_CONTACT_I32 * 4);
    HIP_TRY(h, hipStreamSynchronize(st));
    return LPVMPC_OK;
}

// one tick on caller-supplied data; one-off device buffers, freed when the call returns
extern "C" int lpvmpc_contact_step_batch(lpvmpc_handle *h, int32_t B, int32_t n_heats, const int32_t *heat, const lpvmpc_heats_config *heats_cfg,
                                         const lpvmpc_interaction_config *cfg, const lpvmpc_contact_config *contact_cfg, int32_t t, double *plant,
                                         const double *plant_params, const int32_t *nstep, double *carry_f64, int32_t *carry_i32,
                                         double *ccarry_f64, int32_t *ccarry_i32, double *mu_live, double *f64, int32_t *i32, double *cf64,
                                         int32_t *ci32) {
    const char *who = "lpvmpc_contact_step_batch";
    if (h && B == 0) return LPVMPC_OK;
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h)) return fail(h, LPVMPC_E_ARG, "%s: this handle runs a fleet, cascade or race; use another handle for batch calls", who);
    if (B < 0 || n_heats < 0 || !heat || !cfg || !contact_cfg || !plant || !plant_params || !carry_f64 || !carry_i32 || !ccarry_f64 || !ccarry_i32 ||
        !mu_live || !f64 || !i32 || !cf64 || !ci32)
        return fail(h, LPVMPC_E_ARG, "%s: B < 0, n_heats < 0 or NULL argument", who);
    int rc = lpvmpc_heat_extents(h, who, heats_cfg); if (rc) return rc;
    rc = lpvmpc_interaction_check_config(h, who, cfg); if (rc) return rc;
    if (!cfg->contact) return fail(h, LPVMPC_E_ARG, "%s: the interactions' configuration has contact = 0: there is no contact to give a form to", who);
    rc = check_config(h, who, contact_cfg); if (rc) return rc;
    std::vector<int32_t> off, members;
    int largest = 0;
    rc = lpvmpc_heat_members(h, who, B, n_heats, heat, off, members, largest); if (rc) return rc;
    std::vector<double> tab;                                                    // [7][B], checked (m > 0, Iz > 0, mu >= 0)
    rc = lpvmpc_plant_rows(h, B, plant_params, h->cfg, 0.0, who, tab); if (rc) return rc;
    const size_t n = B;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;
    lpvmpc::ContactDev d{};
    lpvmpc::InterDev &e = d.i;
    double *d_m = nullptr, *d_base = nullptr, *d_iz = nullptr;
    int32_t *d_off = nullptr, *d_members = nullptr, *d_nstep = nullptr;
    hipError_t err = hipSuccess;
    auto take = [&](auto *&p, size_t bytes) { if (err == hipSuccess) err = mem.alloc(p, bytes ? bytes : 8); };
    take(d_off, off.size() * 4); take(d_members, members.size() * 4); take(e.plant, n * 8 * 8); take(d_m, n * 8); take(d_base, n * 8);
    take(d_iz, n * 8); take(e.mu_live, n * 8);
    if (nstep) take(d_nstep, n * 4);
    take(e.carry_f, n * LPVMPC_INTER_CARRY_F64 * 8); take(e.carry_i, n * LPVMPC_INTER_CARRY_I32 * 4);
    take(e.out_f, n * LPVMPC_INTER_F64 * 8); take(e.out_i, n * LPVMPC_INTER_I32 * 4);
    take(d.carry_f, n * LPVMPC_CONTACT_CARRY_F64 * 8); take(d.carry_i, n * LPVMPC_CONTACT_CARRY_I32 * 4);
    take(d.out_f, n * LPVMPC_CONTACT_F64 * 8); take(d.out_i, n * LPVMPC_CONTACT_I32 * 4);
    if (err != hipSuccess) return fail(h, LPVMPC_E_NOMEM, "%s: hipMalloc failed: %s", who, hipGetErrorString(err));
    e.B = B; e.n_heats = n_heats; e.hl = heats_cfg->half_length; e.hwc = heats_cfg->half_width_car;
    e.off = d_off; e.members = d_members; e.nstep = d_nstep; e.m = d_m; e.mu_base = d_base;
    lpvmpc_interaction_set_config(*cfg, e);
    d.friction = contact_cfg->friction; d.yaw_response = contact_cfg->yaw_response; d.Iz = d_iz;
    std::vector<double> f, kf;
    std::vector<int32_t> i, ki;
    lpvmpc_interaction_blank_outputs(n, heat, tab.data() + 6 * n, f, i);
    blank_outputs(n, heat, kf, ki);
    hipStream_t st = h->stream;
    auto run = [&]() -> int {
        H2D(d_off, off.data(), off.size() * 4);
        if (!members.empty()) H2D(d_members, members.data(), members.size() * 4);
        H2D(e.plant, plant, n * 8 * 8); H2D(d_m, tab.data() + 2 * n, n * 8); H2D(d_iz, tab.data() + 3 * n, n * 8);
        H2D(d_base, tab.data() + 6 * n, n * 8); H2D(e.mu_live, tab.data() + 6 * n, n * 8);
        if (nstep) H2D(d_nstep, nstep, n * 4);
        H2D(e.carry_f, carry_f64, n * LPVMPC_INTER_CARRY_F64 * 8); H2D(e.carry_i, carry_i32, n * LPVMPC_INTER_CARRY_I32 * 4);
        H2D(d.carry_f, ccarry_f64, n * LPVMPC_CONTACT_CARRY_F64 * 8); H2D(d.carry_i, ccarry_i32, n * LPVMPC_CONTACT_CARRY_I32 * 4);
        H2D(e.out_f, f.data(), f.size() * 8); H2D(e.out_i, i.data(), i.size() * 4);
        H2D(d.out_f, kf.data(), kf.size() * 8); H2D(d.out_i, ki.data(), ki.size() * 4);
        HIP_TRY(h, lpvmpc::launch_contact_tick(d, largest <= 64 ? 64 : 256, t, st));
        D2H(plant, e.plant, n * 8 * 8); D2H(mu_live, e.mu_live, n * 8);
        D2H(carry_f64, e.carry_f, n * LPVMPC_INTER_CARRY_F64 * 8); D2H(carry_i32, e.carry_i, n * LPVMPC_INTER_CARRY_I32 * 4);
        D2H(ccarry_f64, d.carry_f, n * LPVMPC_CONTACT_CARRY_F64 * 8); D2H(ccarry_i32, d.carry_i, n * LPVMPC_CONTACT_CARRY_I32 * 4);
        D2H(f64, e.out_f, f.size() * 8); D2H(i32, e.out_i, i.size() * 4);
        D2H(cf64, d.out_f, kf.size() * 8); D2H(ci32, d.out_i, ki.size() * 4);
        HIP_TRY(h, hipStreamSynchronize(st));
        return LPVMPC_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);                                             // nothing in flight reads the buffers when they are freed
    return rc;
}
