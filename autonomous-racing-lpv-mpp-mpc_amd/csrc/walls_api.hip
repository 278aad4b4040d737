// walls_api.hip -- C ABI of the walls (include/lpvmpc.h, "Walls"): attaching them to a race, reading the outputs, and the stand-alone
// tick on caller-supplied data.  Kernel: walls.hip.  The binding lives in the race (race_api.hip owns the slot and launches the tick's
// kernel behind the disturbances' and the interactions'); it is built in a local and installed only when it is whole.
#include <cmath>
#include <new>
#include <vector>

#include "walls_host.hpp"

namespace {

int check_config(lpvmpc_handle *h, const char *who, const lpvmpc_wall_config *c) {
    const double w[7] = {c->margin, c->reach, c->half_length, c->half_width_car, c->restitution, c->friction, c->push};
    for (double v : w)
        if (!std::isfinite(v)) return fail(h, LPVMPC_E_ARG, "%s: a word of the configuration is not finite", who);
    if (c->margin < 0 || !(c->reach > 0) || !(c->half_length > 0) || !(c->half_width_car > 0) || c->restitution < 0 || c->restitution > 1 ||
        c->friction < 0 || c->push < 0 || c->push > 1 || (c->yaw_response != 0 && c->yaw_response != 1))
        return fail(h, LPVMPC_E_ARG, "%s: margin = %g, reach = %g, half_length = %g, half_width_car = %g, restitution = %g, friction = %g, push = %g, "
                    "yaw_response = %d (margin, friction >= 0; reach, half_length, half_width_car > 0; restitution, push in [0, 1]; yaw_response 0 / 1)",
                    who, c->margin, c->reach, c->half_length, c->half_width_car, c->restitution, c->friction, c->push, c->yaw_response);
    if (c->reserved != 0) return fail(h, LPVMPC_E_ARG, "%s: reserved = %d must be 0", who, c->reserved);
    return LPVMPC_OK;
}

void set_config(const lpvmpc_wall_config &c, lpvmpc::WallDev &d) {
    d.margin = c.margin; d.reach = c.reach; d.hl = c.half_length; d.hwc = c.half_width_car; d.restitution = c.restitution;
    d.friction = c.friction; d.push = c.push; d.yaw_response = c.yaw_response;
}

// the track a corner is located on: the handle's binding, else its own table in the device copy of its configuration
void set_track(const lpvmpc_handle *h, double hw, lpvmpc::WallDev &d) {
    d.trk = h->trk;
    d.tab = h->d_cfg->track;                                                    // (an address in device memory: nothing is read here)
    d.rows = h->dev.track_rows;
    d.hw = hw;
}

// what a vehicle reads before its first tick: zeros, no corner, no first hit
void blank_outputs(size_t B, std::vector<double> &f, std::vector<int32_t> &i, std::vector<int32_t> &ci) {
    f.assign(B * LPVMPC_WALL_F64, 0.0);
    i.assign(B * LPVMPC_WALL_I32, 0);
    ci.assign(B * LPVMPC_WALL_CARRY_I32, 0);
    for (size_t b = 0; b < B; ++b) {
        i[(size_t)LPVMPC_WALL_CORNER * B + b] = -1; i[(size_t)LPVMPC_WALL_FIRST_HIT_TICK * B + b] = -1;
        ci[(size_t)LPVMPC_WALL_CARRY_FIRST_HIT_TICK * B + b] = -1;
    }
}

}  // namespace

extern "C" void lpvmpc_wall_default_config(lpvmpc_wall_config *c) {
    if (!c) return;
    // invented values of the right order for a 1:10 car on a track of half width 0.3: nothing in the reference fixes them
    c->margin = 0.25; c->reach = 0.5; c->half_length = 0.4; c->half_width_car = 0.2; c->restitution = 0.2; c->friction = 0.3; c->push = 0.5;
    c->yaw_response = 1; c->reserved = 0;
}

extern "C" int lpvmpc_race_walls(lpvmpc_handle *h, const lpvmpc_wall_config *cfg) {
    const char *who = "lpvmpc_race_walls";
    RaceAttach a;
    RC_TRY(a.begin(h, who));
    const RaceAttachView &v = a.v;
    hipStream_t st = a.st;
    if (!cfg) return lpvmpc_race_detach(h, RACE_WALLS);
    if (!v.side->veh.d.p)
        return fail(h, LPVMPC_E_ARG, "%s: the race has no plant table (start it through lpvmpc_race_init_vehicles / lpvmpc_race_init_tyres): there is "
                    "no mass and no yaw inertia to answer an impulse with", who);
    RC_TRY(check_config(h, who, cfg));
    std::unique_ptr<WallBinding> q(new (std::nothrow) WallBinding());           // installed once it is complete
    if (!q) return fail(h, LPVMPC_E_NOMEM, "out of host memory");
    const size_t B = v.B;
    const double *live = v.side->veh.d.p;                                       // [7][B]
    lpvmpc::WallDev &e = q->d;
    const Planes pl = lpvmpc_wall_planes(e, B);
    DevTake take{q->mem};
    pl.alloc(take);
    RC_TRY(take.check(h, who, true));
    e.B = v.B;
    set_track(h, v.hw, e);
    set_config(*cfg, e);
    e.plant = v.plant; e.nstep = v.nstep; e.m = live + 2 * B; e.Iz = live + 3 * B;
    q->cfg = *cfg;
    std::vector<double> f;
    std::vector<int32_t> i, ci;
    blank_outputs(B, f, i, ci);
    return lpvmpc_race_install(h, st, *v.walls, q, [&]() -> int {              // (its synchronisation: no tick in flight reads the old binding)
        RC_TRY(pl.blank_carry(h, st, ci.data()));
        return pl.blank_out(h, st, f, i);
    }, v.walls_serial);
}

static Planes read_planes(WallBinding &q) { return lpvmpc_wall_planes(q.d, q.d.B); }

extern "C" int lpvmpc_race_walls_read(lpvmpc_handle *h, double *f64, int32_t *i32) {
    return lpvmpc_race_read_planes(h, "lpvmpc_race_walls_read", &RaceAttachView::walls, "no walls are attached (lpvmpc_race_walls)", read_planes, f64,
                                   i32);
}

// one tick on caller-supplied data; one-off device buffers, freed when the call returns
extern "C" int lpvmpc_wall_step_batch(lpvmpc_handle *h, int32_t B, const lpvmpc_wall_config *cfg, double half_width, int32_t t, double *plant,
                                      const double *plant_params, const int32_t *nstep, double *carry_f64, int32_t *carry_i32, double *f64,
                                      int32_t *i32) {
    const char *who = "lpvmpc_wall_step_batch";
    int rc;
    if (lpvmpc_batch_done(h, B, who, rc)) return rc;
    if (B < 0 || !cfg || !plant || !plant_params || !carry_f64 || !carry_i32 || !f64 || !i32)
        return fail(h, LPVMPC_E_ARG, "%s: B < 0 or NULL argument", who);
    RC_TRY(lpvmpc_need_track(h, who));
    RC_TRY(lpvmpc_tracks_check(h, B, who));
    if (!h->trk.tab && !(std::isfinite(half_width) && half_width >= 0))
        return fail(h, LPVMPC_E_ARG, "%s: half_width = %g must be finite and >= 0", who, half_width);
    RC_TRY(check_config(h, who, cfg));
    std::vector<double> tab;                                                    // [7][B], checked (m > 0, Iz > 0)
    RC_TRY(lpvmpc_plant_rows(h, B, plant_params, h->cfg, 0.0, who, tab));
    const size_t n = B;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    DevArena mem;
    lpvmpc::WallDev e{};
    const Planes pl = lpvmpc_wall_planes(e, n);
    double *d_m = nullptr, *d_Iz = nullptr;
    int32_t *d_nstep = nullptr;
    DevTake take{mem};
    take(e.plant, n * 8 * 8); take(d_m, n * 8); take(d_Iz, n * 8);
    if (nstep) take(d_nstep, n * 4);
    pl.alloc(take);
    RC_TRY(take.check(h, who, false));
    e.B = B; e.nstep = d_nstep; e.m = d_m; e.Iz = d_Iz;
    set_track(h, half_width, e);
    set_config(*cfg, e);
    hipStream_t st = h->stream;
    return lpvmpc_run_synced(h, st, [&]() -> int {                              // nothing in flight reads the buffers when they are freed
        H2D(e.plant, plant, n * 8 * 8); H2D(d_m, tab.data() + 2 * n, n * 8); H2D(d_Iz, tab.data() + 3 * n, n * 8);
        if (nstep) H2D(d_nstep, nstep, n * 4);
        RC_TRY(pl.carry_in(h, st, carry_f64, carry_i32));
        HIP_TRY(h, lpvmpc::launch_wall_tick(e, t, st));                        // (every vehicle's output words are written by its quad)
        D2H(plant, e.plant, n * 8 * 8);
        return pl.copy_out(h, st, carry_f64, carry_i32, f64, i32);
    });
}
