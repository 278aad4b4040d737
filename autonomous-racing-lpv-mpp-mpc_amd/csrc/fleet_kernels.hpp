// fleet_kernels.hpp -- the fleet kernels that advance a plant, each in its plain form (kAct = false: closed_loop.hip, observer.hip,
// race.hip) and its delayed form (kAct = true: actuator.hip).  One lane per vehicle, as closed_loop.hip.  The delayed form steps the
// plant through the actuator stage (act_stage, track_geometry.hpp: motor / steering FIFOs and the servo filter, vehicleSimulator.py:
// 53-78) and keeps the controller's OldSteering / OldAccelera history of steering delay sd (uold_push, controllerMain.py:289-298)
// where the plain form writes the last command.  Its estimator kernels feed the observer the COMMANDED input (it subscribes to `ecu`,
// stateEstimator.py:785) and the plant the actuator stage's output.  The plain forms take (and ignore) sd and ActDev.
//
// Five of them -- the kernels that step the plant -- have a per-vehicle form (kVeh = true, always with kAct = true): their plant
// argument is the fleet's table of per-vehicle parameters (VehPlantCfg, PlantArg<kVeh>) instead of one PlantCfg, and each simulator
// step reads the vehicle's row (plant_step_at, track_geometry.hpp).  kVeh defaults to false, so the plain and delayed forms keep
// their code.  The same five have a tyre form (kTyre = true, always with kVeh = true): the argument is the plant table plus the
// fleet's tyre table (TyrePlantCfg), and plant_step_at takes the vehicle's tyre row as well (linear or Pacejka, per vehicle).
//
// The two estimator kernels among them have a per-vehicle-estimator form on top (kObsVeh = true, always with kVeh = true): their
// `gains` argument carries the binding's model rows and gain planes (ObsGainsArg<true>, observer_device.hpp), and each observer
// step reads the vehicle's row and its own gain words; observer_vehicles.hip instantiates them, with and without the tyre table.
//
// One instantiation per translation unit: the .hip files above instantiate <false> only, actuator.hip <true> only, plant_params.hip
// <true, true> only, tyre.hip <true, true, true> only.  With both
// forms of a kernel in one translation unit LLVM compiles the plain form differently (other registers, other instructions); with
// one per translation unit each form compiles to the code it has alone (docs/HISTORY.md, "Fleet kernels as templates").
// tests/test_fleet_kernel_instances.py guards the rule.
//
// Each launcher stands next to its instantiation and takes its family's argument struct (lpvmpc_device.hpp: FleetStepArgs ...).
// Which form serves an engine is decided away from the kernels: step_form.hpp maps the engine's form to a kernel enumerator, and
// fleet_launch.hip binds the enumerators to the launchers.
#pragma once
#include "lpvmpc_device.hpp"
#include "observer_device.hpp"
#include "track_geometry.hpp"

namespace lpvmpc {

// Some of the kernels that read the track share their body with a bound form on per-vehicle tracks (track_vehicles.hip).  Kernel
// arguments differ between the two, so the kernels stay apart; the body is a function template over the track source `src`
// (track_geometry.hpp, track_view), forced inline and instantiated once per object.  Which pairs share is decided by the device code:
// a pair whose kernels do not all keep their instruction stream stays restated, with the measurement in its comment ("One
// source, one form per object").

// the stand-alone transforms of vehicle b (closed_loop.hip, track_vehicles.hip): in [B][3] -> out [B][4], in [B][2] -> out [B][3]
template <class Src>
__device__ __forceinline__ void local_position_body(const Src &src, double hw, double slack, int b, const double *in, double *out) {
    const auto &v = track_view(src, b, hw, slack);
    double s, ey, epsi; int inside;
    local_position(v, hw, slack, in[b * 3 + 0], in[b * 3 + 1], in[b * 3 + 2], s, ey, epsi, inside);
    out[b * 4 + 0] = s; out[b * 4 + 1] = ey; out[b * 4 + 2] = epsi; out[b * 4 + 3] = inside;
}
template <class Src>
__device__ __forceinline__ void global_position_body(const Src &src, int b, const double *in, double *out) {
    double x, y, th;
    global_position(track_view(src, b), in[b * 2 + 0], in[b * 2 + 1], x, y, th);
    out[b * 3 + 0] = x; out[b * 3 + 1] = y; out[b * 3 + 2] = th;
}

// n_sub simulator steps under u = [motor, servo] per vehicle (lpvmpc_plant_step_batch / _actuated_batch)
template <bool kAct, bool kVeh = false, bool kTyre = false>
__global__ void __launch_bounds__(64) plant_kernel(int B, double *__restrict__ plant, const double *__restrict__ u, PlantArg<kVeh, kTyre> pc, ActDev a) {
    static_assert((kAct || !kVeh) && (kVeh || !kTyre), "the per-vehicle forms are delayed forms, the tyre forms per-vehicle forms");
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
    const double motor = u[b * 2 + 0], servo = u[b * 2 + 1];
    if constexpr (kAct) {
        const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
        double sv = a.servo[b];
        for (int k = 0; k < pc.n_sub; ++k) {
            double ua, ud;
            act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
            plant_step_at(pc, b, st, ua, ud);
        }
        a.k[b] = k0 + pc.n_sub; a.servo[b] = sv;
    } else {
        for (int k = 0; k < pc.n_sub; ++k) plant_step(pc, st, motor, servo);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
}

// lap-0 measurement: GlobalState = [vx vy psiDot x y psi] from the plant (ground truth), vx clamped at 0.01
// (CMAIN:183-184), local coordinates from the map.  q9_swap reproduces CMAIN:188, which stores the returned
// (s, ey, epsi) as LocalState[4], LocalState[3], LocalState[5], i.e. ey lands in the epsi slot and vice versa
// (SURVEY quirk Q9); with q9_swap = 0 the slots are filled as the state definition says.
// u_old = last command [servo, motor] (CMAIN:289-298 leaves exactly that in OldSteering[0] / OldAccelera[0]).
// The delayed form's body, shared with cl_measure_trk_kernel.  The plain form keeps its two statements in the kernel: through this body
// (with kAct as a flag) cl_measure_kernel<false> of closed_loop.o kept its 1638 instructions but had three of them scheduled elsewhere
template <class Src>
__device__ __forceinline__ void cl_measure_body(const Src &src, int b, const double *plant, const double *cmd, double hw, double slack, int q9_swap,
                                                double *local_state, double *u_old, int sd) {
    const auto &v = track_view(src, b, hw, slack);
    cl_local(v, hw, slack, q9_swap, plant + (size_t)b * 8, local_state + (size_t)b * 6);
    uold_push(u_old + (size_t)b * (2 + sd), sd, cmd[b * 2 + 0], cmd[b * 2 + 1]);
}
template <bool kAct>
__global__ void __launch_bounds__(64) cl_measure_kernel(const DevCfg *__restrict__ cp, int B, const double *__restrict__ plant,
                                                        const double *__restrict__ cmd, double hw, double slack, int q9_swap,
                                                        double *__restrict__ local_state, double *__restrict__ u_old, int sd) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if constexpr (kAct) cl_measure_body(*cp, b, plant, cmd, hw, slack, q9_swap, local_state, u_old, sd);
    else {
        cl_local(*cp, hw, slack, q9_swap, plant + (size_t)b * 8, local_state + (size_t)b * 6);
        u_old[b * 2 + 0] = cmd[b * 2 + 0]; u_old[b * 2 + 1] = cmd[b * 2 + 1];
    }
}

// command = first predicted input (CMAIN:381-386: servo = uPred[0,0], motor = uPred[0,1]), n_sub simulator steps under it
// (u = [motor, servo], vehicleSimulator.py:330), then the NEXT tick's measurement (cl_measure_kernel on the state just advanced):
// one launch less per control tick; the measurement goes to its own buffer, the previous tick's local state stays readable
template <bool kAct, bool kVeh = false, bool kTyre = false>
__global__ void __launch_bounds__(64) cl_command_plant_measure_kernel(const DevCfg *__restrict__ cp, int B, int N, const double *__restrict__ uPred,
                                                                      double *__restrict__ cmd, double *__restrict__ plant, PlantArg<kVeh, kTyre> pc,
                                                                      double hw, double slack, int q9_swap, double *__restrict__ local_next,
                                                                      double *__restrict__ u_old, int sd, ActDev a) {
    static_assert((kAct || !kVeh) && (kVeh || !kTyre), "the per-vehicle forms are delayed forms, the tyre forms per-vehicle forms");
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double servo = uPred[(size_t)b * N * 2 + 0], motor = uPred[(size_t)b * N * 2 + 1];
    cmd[b * 2 + 0] = servo; cmd[b * 2 + 1] = motor;
    double st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
    if constexpr (kAct) {
        const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
        double sv = a.servo[b];
        for (int k = 0; k < pc.n_sub; ++k) {
            double ua, ud;
            act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
            plant_step_at(pc, b, st, ua, ud);
        }
        a.k[b] = k0 + pc.n_sub; a.servo[b] = sv;
    } else {
        for (int k = 0; k < pc.n_sub; ++k) plant_step(pc, st, motor, servo);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
    // the next tick's measurement, cl_local.  The plain form has it written out, with the output pointer formed after local_position:
    // in that order the plain form keeps its code, in cl_local's the delayed form does (the other order costs each form SGPR spills)
    if constexpr (kAct) {
        cl_local(*cp, hw, slack, q9_swap, st, local_next + (size_t)b * 6);
        uold_push(u_old + (size_t)b * (2 + sd), sd, servo, motor);
    } else {
        double s, ey, epsi; int inside;
        local_position(*cp, hw, slack, st[0], st[1], st[6], s, ey, epsi, inside);
        double *ls = local_next + (size_t)b * 6;
        ls[0] = st[2] < 0.01 ? 0.01 : st[2]; ls[1] = st[3]; ls[2] = st[7];
        ls[3] = q9_swap ? ey : epsi; ls[4] = s; ls[5] = q9_swap ? epsi : ey;
        u_old[b * 2 + 0] = servo; u_old[b * 2 + 1] = motor;
    }
}

// cl_command_plant_measure_kernel with the estimator in the loop: per plant step, plant -> sensors -> observer; the next tick's
// measurement is made from the estimate.  mode 0: only the measurement of the current estimate with u_old = cmd (the first
// tick of a fleet; one kernel keeps local_position at a single call site, inlined).  mode 2 (the cascade, plain form only):
// advance, then write the estimate in the plant's layout [x y vx vy 0 0 yaw psiDot] to local_next [B][8], which the cascade's
// measurement kernels read in place of the plant; u_old is left to them
template <bool kAct, bool kVeh = false, bool kTyre = false, bool kObsVeh = false>
__global__ void __launch_bounds__(64) cl_command_plant_observe_kernel(const DevCfg *__restrict__ cp, int B, int N, const double *__restrict__ uPred,
                                                                      double *__restrict__ cmd, double *__restrict__ plant, PlantArg<kVeh, kTyre> pc,
                                                                      double hw, double slack, int q9_swap, double *__restrict__ local_next,
                                                                      double *__restrict__ u_old, typename ObsGainsArg<kObsVeh>::type gains,
                                                                      double *__restrict__ obs, ObsParams op, int mode, int sd, ActDev a) {
    static_assert((kAct || !kVeh) && (kVeh || !kTyre), "the per-vehicle forms are delayed forms, the tyre forms per-vehicle forms");
    static_assert(kVeh || !kObsVeh, "the per-vehicle estimator runs in the per-vehicle forms");
    __shared__ double G[kObsGainWords];
    if (mode != 0) obs_stage_gains(G, obs_gain_words(gains));
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double os[kObsStride];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) os[i] = obs[(size_t)b * kObsStride + i];
    double servo = cmd[b * 2 + 0], motor = cmd[b * 2 + 1];
    if (mode != 0) {
        servo = uPred[(size_t)b * N * 2 + 0]; motor = uPred[(size_t)b * N * 2 + 1];
        cmd[b * 2 + 0] = servo; cmd[b * 2 + 1] = motor;
        double st[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
        const long long vid = op.voff + b;
        int k0 = 0, La = 0, Ld = 0;
        double sv = 0.0;
        if constexpr (kAct) { k0 = a.k[b]; La = a.La[b]; Ld = a.Ld[b]; sv = a.servo[b]; }
        for (int k = 0; k < pc.n_sub; ++k) {
            if constexpr (kAct) {
                // compiler-only barrier, as in race_command_plant_observe_kernel: keeps the gain words' LDS loads inside the loop
                // (the plain form has never had it)
                asm volatile("" ::: "memory");
                double ua, ud;
                act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
                plant_step_at(pc, b, st, ua, ud);
            } else {
                plant_step(pc, st, motor, servo);
            }
            obs_substep<kObsVeh>(G, op, vid, os, st, servo, motor, obs_veh(gains), b);
        }
        if constexpr (kAct) { a.k[b] = k0 + pc.n_sub; a.servo[b] = sv; }
#pragma unroll
        for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
#pragma unroll
        for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
    }
    if constexpr (!kAct) {
        if (mode == 2) {
            double *v = local_next + (size_t)b * 8;
            v[0] = os[3]; v[1] = os[4]; v[2] = os[0]; v[3] = os[1]; v[4] = 0.0; v[5] = 0.0; v[6] = os[5]; v[7] = os[2];
            return;
        }
    }
    obs_local_state(*cp, hw, slack, q9_swap, os, local_next + (size_t)b * 6);
    if constexpr (kAct) uold_push(u_old + (size_t)b * (2 + sd), sd, servo, motor);
    else { u_old[b * 2 + 0] = servo; u_old[b * 2 + 1] = motor; }
}

// measurement (from r.meas), lap logic and this tick's controller masks.  c is the controllers' configuration (path and TT share
// N, dt, track).  A vehicle entering the tick with a non-finite plant or measurement source is lost.
// seed_tick: the race's first 9 ticks (first_it < 10, CMAIN:310-320) solve the path controller on the seed trajectories.
template <bool kAct>
__global__ void __launch_bounds__(64) race_measure_kernel(const DevCfg *__restrict__ cp, RaceDev r, int seed_tick, int sd) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= r.B) return;
    const int N = c.N, M = r.M;
    r.m_path[b] = 0; r.m_tt[b] = 0; r.nstep[b] = 0; r.src[b] = -1;
    const int ph = r.phase[b];
    if (ph >= 2) return;                                                    // finished / lost: frozen
    const double *p = r.meas + (size_t)b * 8;
    if (!plant_finite(r.plant + (size_t)b * 8) || !plant_finite(p)) { r.phase[b] = 3; return; }
    r.alive[b] += 1;
    const double L = c.track[(c.track_rows - 1) * 6 + 3] + c.track[(c.track_rows - 1) * 6 + 4];
    double *ls = r.local + (size_t)b * 6;
    bool event = false;
    int k = 0;
    if (ph == 0) {                                                          // CMAIN:186-190
        cl_local(c, r.hw, r.slack, r.q9, p, ls);
        if (ls[4] >= 3 * L / 4) r.half[b] = 1;
        if (r.half[b] == 1 && ls[4] <= L / 4) {                             // CMAIN:254-262: lap event
            r.half[b] = 0; r.lap[b] = 1; r.SSc[b] = 0.0; r.phase[b] = 1;
            r.rk[b] = 0; r.plan_done[b] = 0; r.idx[b] = 0;
            for (int i = 0; i <= r.Np; ++i) r.SSp[(size_t)b * (r.Np + 1) + i] = 0.0;     // the planner node starts (PMAIN:72-74,124)
            r.pose[b * 3 + 0] = r.pose[b * 3 + 1] = r.pose[b * 3 + 2] = 0.0;
            if (1 < r.lap_cols) r.lap_step[(size_t)b * r.lap_cols + 1] = r.step[b];
            event = true;
        }
    } else {                                                                // CMAIN:198-248, 266-279
        k = r.rk[b];
        if (r.idx[b] == 0) {                                                // `index` toggle: re-read the windows on racing ticks 0, 2, 4, ...
            const double *m = r.refs + (size_t)b * 5 * M;
            for (int i = 0; i < N; ++i) { r.t_vel[(size_t)b * (N + 1) + i] = m[3 * M + i]; r.t_curv[(size_t)b * N + i] = m[4 * M + i]; }
            r.t_vel[(size_t)b * (N + 1) + N] = m[3 * M + N - 1];
            r.ref0[b * 3 + 0] = m[0]; r.ref0[b * 3 + 1] = m[M]; r.ref0[b * 3 + 2] = m[2 * M];
            r.idx[b] = 1;
        } else r.idx[b] = 0;
        const int lp = r.lap[b];
        tt_local(c, p, lp, r.ref0 + b * 3, r.t_curv[(size_t)b * N], r.SSc[b], ls);
        const double s = ls[4];
        if (fabs(p[0]) < 0.1 && s >= L - L / 10) {
            r.lap[b] = lp + 1; r.SSc[b] = 0.0;
            if (lp + 1 < r.lap_cols) r.lap_step[(size_t)b * r.lap_cols + lp + 1] = r.step[b];
            if (lp + 1 > r.laps) { r.phase[b] = 2; return; }                // RunController = 0: nothing of this tick is applied
        } else r.SSc[b] = s;
        r.rk[b] = k + 1;
    }
    const int lap = r.lap[b];
    double *uo = lap == 0 ? r.p_uold : r.t_uold;                            // CMAIN:289-298: the controller of the vehicle's lap
    if constexpr (kAct) uold_push(uo + (size_t)b * (2 + sd), sd, r.cmd[b * 2 + 0], r.cmd[b * 2 + 1]);
    else { uo[b * 2 + 0] = r.cmd[b * 2 + 0]; uo[b * 2 + 1] = r.cmd[b * 2 + 1]; }
    if (seed_tick || lap == 0) {
        r.m_path[b] = 1; r.src[b] = 0;
    } else {
        r.m_tt[b] = 1; r.src[b] = 1;
        if (event) {                                                        // CMAIN:326-327,336,361-363 on the event tick
            for (int i = 0; i <= N; ++i) r.t_vel[(size_t)b * (N + 1) + i] = 1.0;
            for (int i = 0; i < N; ++i) r.t_curv[(size_t)b * N + i] = 0.0;
            for (int i = 0; i < 2 * N; ++i) r.t_uPred[(size_t)b * N * 2 + i] = r.p_uPred[(size_t)b * N * 2 + i];
        }
    }
    r.nstep[b] = ph == 0 ? r.n_sub_lap0 : r.n_sub[k % 3];
}

// last launch of a tick: the solve's report, the command of the vehicle's controller and its simulator steps.  A frozen vehicle
// (nstep 0) advances neither plant nor actuator
template <bool kAct, bool kVeh = false, bool kTyre = false>
__global__ void __launch_bounds__(64) race_command_plant_kernel(RaceDev r, PlantArg<kVeh, kTyre> pc, ActDev a) {
    static_assert((kAct || !kVeh) && (kVeh || !kTyre), "the per-vehicle forms are delayed forms, the tyre forms per-vehicle forms");
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= r.B) return;
    const int src = r.src[b], n = r.nstep[b], N = r.N;
    if (src == 0) { r.iters[b] = r.p_iters[b]; r.status[b] = r.p_status[b]; }
    else if (src == 1) { r.iters[b] = r.t_iters[b]; r.status[b] = r.t_status[b]; }
    else r.iters[b] = 0;
    if (n == 0) return;
    const double *u = (r.lap[b] == 0 ? r.p_uPred : r.t_uPred) + (size_t)b * N * 2;
    const double servo = u[0], motor = u[1];
    r.cmd[b * 2 + 0] = servo; r.cmd[b * 2 + 1] = motor;
    double st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = r.plant[(size_t)b * 8 + i];
    if constexpr (kAct) {
        const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
        double sv = a.servo[b];
        for (int k = 0; k < n; ++k) {
            double ua, ud;
            act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
            plant_step_at(pc, b, st, ua, ud);
        }
        a.k[b] = k0 + n; a.servo[b] = sv;
    } else {
        for (int k = 0; k < n; ++k) plant_step(pc, st, motor, servo);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) r.plant[(size_t)b * 8 + i] = st[i];
    r.step[b] += n;
}

// race_command_plant_kernel with the estimator in the loop: per plant step, plant -> sensors -> observer (obs_substep, the schedule
// of cl_command_plant_observe_kernel), then the estimate view that the next tick's measurements read.  A frozen vehicle (nstep 0)
// advances neither the plant, its actuator nor its observer, so its noise keys (vid, step) depend on its own steps only.
template <bool kAct, bool kVeh = false, bool kTyre = false, bool kObsVeh = false>
__global__ void __launch_bounds__(64) race_command_plant_observe_kernel(RaceDev r, PlantArg<kVeh, kTyre> pc, typename ObsGainsArg<kObsVeh>::type gains,
                                                                        double *__restrict__ obs, ObsParams op, ActDev a) {
    static_assert((kAct || !kVeh) && (kVeh || !kTyre), "the per-vehicle forms are delayed forms, the tyre forms per-vehicle forms");
    static_assert(kVeh || !kObsVeh, "the per-vehicle estimator runs in the per-vehicle forms");
    __shared__ double G[kObsGainWords];
    obs_stage_gains(G, obs_gain_words(gains));
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= r.B) return;
    const int src = r.src[b], n = r.nstep[b], N = r.N;
    if (src == 0) { r.iters[b] = r.p_iters[b]; r.status[b] = r.p_status[b]; }
    else if (src == 1) { r.iters[b] = r.t_iters[b]; r.status[b] = r.t_status[b]; }
    else r.iters[b] = 0;
    if (n == 0) return;
    const double *u = (r.lap[b] == 0 ? r.p_uPred : r.t_uPred) + (size_t)b * N * 2;
    const double servo = u[0], motor = u[1];
    r.cmd[b * 2 + 0] = servo; r.cmd[b * 2 + 1] = motor;
    double st[8], os[kObsStride];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = r.plant[(size_t)b * 8 + i];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) os[i] = obs[(size_t)b * kObsStride + i];
    const long long vid = op.voff + b;
    int k0 = 0, La = 0, Ld = 0;
    double sv = 0.0;
    if constexpr (kAct) { k0 = a.k[b]; La = a.La[b]; Ld = a.Ld[b]; sv = a.servo[b]; }
    for (int k = 0; k < n; ++k) {
        // compiler-only barrier: without it the gain words' LDS loads (read-only after the staging barrier) are hoisted out of
        // the loop for both polytopes, 1968 registers' worth, and spill to scratch (6.7 KB per lane)
        asm volatile("" ::: "memory");
        if constexpr (kAct) {
            double ua, ud;
            act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
            plant_step_at(pc, b, st, ua, ud);
        } else {
            plant_step(pc, st, motor, servo);
        }
        obs_substep<kObsVeh>(G, op, vid, os, st, servo, motor, obs_veh(gains), b);
    }
    if constexpr (kAct) { a.k[b] = k0 + n; a.servo[b] = sv; }
#pragma unroll
    for (int i = 0; i < 8; ++i) r.plant[(size_t)b * 8 + i] = st[i];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
    double *v = r.estv + (size_t)b * 8;
    v[0] = os[3]; v[1] = os[4]; v[2] = os[0]; v[3] = os[1]; v[4] = 0.0; v[5] = 0.0; v[6] = os[5]; v[7] = os[2];
    r.step[b] += n;
}

// the tyre curve alone (lpvmpc_tyre_force_batch): a template like the fleet kernels, so that only tyre.hip holds its code
template <bool kTyre>
__global__ void __launch_bounds__(64) tyre_force_kernel(int B, const double *__restrict__ tyre, const double *__restrict__ m,
                                                        const double *__restrict__ alpha, double *__restrict__ force) {
    static_assert(kTyre, "tyre.hip's kernel");
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double ty[kTyreWords];
#pragma unroll
    for (int i = 0; i < kTyreWords; ++i) ty[i] = tyre[(size_t)i * B + b];
    force[b] = tyre_force(ty, m[b], 60.0, alpha[b]);                        // a linear row: Simulator.f's 60
}

}  // namespace lpvmpc
