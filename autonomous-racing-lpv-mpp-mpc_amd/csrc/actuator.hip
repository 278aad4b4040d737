// actuator.hip -- the reference simulator's actuator model on the device (include/lpvmpc.h, "Actuator delay and servo lag") and the
// delayed forms of the fleet kernels that advance a plant.  One lane per vehicle, as closed_loop.hip.
//
// Replaces, per vehicle:
//   vehicleSimulator.py:53-78    motor / steering FIFOs of int(delay_a / dt) and int(delay_df / dt) zeros, the low-level servo
//                                filter (Tf = 0.07 s) on the delayed steering (act_stage, track_geometry.hpp)
//   controllerMain.py:289-298    OldSteering / OldAccelera of a controller with steeringDelay d: append the last command, drop
//                                the oldest entry (uold_push, track_geometry.hpp)
//
// Each kernel here is the delayed form of a kernel of closed_loop.hip, observer.hip or race.hip and is kept in this object so that
// those kernels compile to the code they had before.  The estimator kernels feed the observer the COMMANDED input (it subscribes to
// `ecu`, stateEstimator.py:785) and the plant the actuator stage's output.
#include "lpvmpc_device.hpp"
#include "observer_device.hpp"
#include "track_geometry.hpp"

namespace lpvmpc {

// plant_kernel through the actuator stage (lpvmpc_plant_step_actuated_batch): n_sub steps under the command u = (motor, servo)
__global__ void __launch_bounds__(64) plant_actuated_kernel(int B, double *__restrict__ plant, const double *__restrict__ u, PlantCfg pc, ActDev a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
    const double motor = u[b * 2 + 0], servo = u[b * 2 + 1];
    const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
    double sv = a.servo[b];
    for (int k = 0; k < pc.n_sub; ++k) {
        double ua, ud;
        act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
        plant_step(pc, st, ua, ud);
    }
    a.k[b] = k0 + pc.n_sub; a.servo[b] = sv;
#pragma unroll
    for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
}

// cl_measure_kernel of the delayed fleet (its first tick): u_old takes the history step
__global__ void __launch_bounds__(64) cl_measure_act_kernel(const DevCfg *__restrict__ cp, int B, const double *__restrict__ plant,
                                                            const double *__restrict__ cmd, double hw, double slack, int q9_swap,
                                                            double *__restrict__ local_state, double *__restrict__ u_old, int sd) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    cl_local(*cp, hw, slack, q9_swap, plant + (size_t)b * 8, local_state + (size_t)b * 6);
    uold_push(u_old + (size_t)b * (2 + sd), sd, cmd[b * 2 + 0], cmd[b * 2 + 1]);
}

// cl_command_plant_measure_kernel (closed_loop.hip) of the delayed lap-0 fleet: the plant steps through the actuator stage, u_old is
// the controller's history of steering delay sd
__global__ void __launch_bounds__(64) cl_command_plant_measure_act_kernel(const DevCfg *__restrict__ cp, int B, int N, const double *__restrict__ uPred,
                                                                          double *__restrict__ cmd, double *__restrict__ plant, PlantCfg pc,
                                                                          double hw, double slack, int q9_swap, double *__restrict__ local_next,
                                                                          double *__restrict__ u_old, int sd, ActDev a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double servo = uPred[(size_t)b * N * 2 + 0], motor = uPred[(size_t)b * N * 2 + 1];
    cmd[b * 2 + 0] = servo; cmd[b * 2 + 1] = motor;
    double st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = plant[(size_t)b * 8 + i];
    const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
    double sv = a.servo[b];
    for (int k = 0; k < pc.n_sub; ++k) {
        double ua, ud;
        act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
        plant_step(pc, st, ua, ud);
    }
    a.k[b] = k0 + pc.n_sub; a.servo[b] = sv;
#pragma unroll
    for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
    cl_local(*cp, hw, slack, q9_swap, st, local_next + (size_t)b * 6);
    uold_push(u_old + (size_t)b * (2 + sd), sd, servo, motor);
}

// the delayed form of cl_command_plant_observe_kernel (cl_command_plant_observe_act_kernel): the plant steps through the actuator
// stage while the observer is fed the COMMANDED (servo, motor), as the estimator subscribes to `ecu` (stateEstimator.py:785); u_old
// is the controller's history of steering delay sd.  Modes 0 and 1 only (the cascade runs on cl_command_plant_observe_kernel).
__device__ __forceinline__ void cl_command_plant_observe_act_body(double *G, const DevCfg *__restrict__ cp, int B, int N, const double *__restrict__ uPred,
                                                                  double *__restrict__ cmd, double *__restrict__ plant, const PlantCfg &pc,
                                                                  double hw, double slack, int q9_swap, double *__restrict__ local_next,
                                                                  double *__restrict__ u_old, double *__restrict__ obs, const ObsParams &op, int mode,
                                                                  int sd, const ActDev &a) {
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
        const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
        double sv = a.servo[b];
        for (int k = 0; k < pc.n_sub; ++k) {
            // compiler-only barrier, as in race_command_plant_observe_kernel: keeps the gain words' LDS loads inside the loop
            asm volatile("" ::: "memory");
            double ua, ud;
            act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
            plant_step(pc, st, ua, ud);
            obs_substep(G, op, vid, os, st, servo, motor);
        }
        a.k[b] = k0 + pc.n_sub; a.servo[b] = sv;
#pragma unroll
        for (int i = 0; i < 8; ++i) plant[(size_t)b * 8 + i] = st[i];
#pragma unroll
        for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
    }
    // the controller's measurement from the estimate, as obs_local_state (observer.hip)
    double s, ey, epsi; int inside;
    local_position(*cp, hw, slack, os[3], os[4], os[5], s, ey, epsi, inside);
    double *ls = local_next + (size_t)b * 6;
    ls[0] = os[0] < 0.01 ? 0.01 : os[0]; ls[1] = os[1]; ls[2] = os[2];
    ls[3] = q9_swap ? ey : epsi; ls[4] = s; ls[5] = q9_swap ? epsi : ey;
    uold_push(u_old + (size_t)b * (2 + sd), sd, servo, motor);
}
// mode 0 (the first tick's measurement) and mode 1 of the delayed lap-0 fleet
__global__ void __launch_bounds__(64) cl_command_plant_observe_act_kernel(const DevCfg *__restrict__ cp, int B, int N, const double *__restrict__ uPred,
                                                                          double *__restrict__ cmd, double *__restrict__ plant, PlantCfg pc,
                                                                          double hw, double slack, int q9_swap, double *__restrict__ local_next,
                                                                          double *__restrict__ u_old, const double *__restrict__ gains,
                                                                          double *__restrict__ obs, ObsParams op, int mode, int sd, ActDev a) {
    __shared__ double G[kObsGainWords];
    if (mode != 0) obs_stage_gains(G, gains);
    cl_command_plant_observe_act_body(G, cp, B, N, uPred, cmd, plant, pc, hw, slack, q9_swap, local_next, u_old, obs, op, mode, sd, a);
}

__device__ inline bool act_plant_finite(const double *p) {
    bool fin = true;
    for (int i = 0; i < 8; ++i) fin = fin && __builtin_isfinite(p[i]);
    return fin;
}

// race_measure_kernel (race.hip) of the delayed race, line for line, except u_old: the controller of the vehicle's lap appends the
// last command to its OldSteering / OldAccelera history (uold_push, steering delay sd).  A copy rather than a template so that the
// original kernel's code stays what it was.
// Measurement (from r.meas), lap logic and this tick's controller masks.  c is the controllers' configuration (path and TT share
// N, dt, track).  A vehicle entering the tick with a non-finite plant or measurement source is lost.
// seed_tick: the race's first 9 ticks (first_it < 10, CMAIN:310-320) solve the path controller on the seed trajectories.
__global__ void __launch_bounds__(64) race_measure_act_kernel(const DevCfg *__restrict__ cp, RaceDev r, int seed_tick, int sd) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= r.B) return;
    const int N = c.N, M = r.M;
    r.m_path[b] = 0; r.m_tt[b] = 0; r.nstep[b] = 0; r.src[b] = -1;
    const int ph = r.phase[b];
    if (ph >= 2) return;                                                    // finished / lost: frozen
    const double *p = r.meas + (size_t)b * 8;
    if (!act_plant_finite(r.plant + (size_t)b * 8) || !act_plant_finite(p)) { r.phase[b] = 3; return; }
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
    uold_push(uo + (size_t)b * (2 + sd), sd, r.cmd[b * 2 + 0], r.cmd[b * 2 + 1]);
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

// race_command_plant_kernel (race.hip) through the actuator stage: a frozen vehicle (nstep 0) advances neither plant nor actuator
__global__ void __launch_bounds__(64) race_command_plant_act_kernel(RaceDev r, PlantCfg pc, ActDev a) {
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
    const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
    double sv = a.servo[b];
    for (int k = 0; k < n; ++k) {
        double ua, ud;
        act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
        plant_step(pc, st, ua, ud);
    }
    a.k[b] = k0 + n; a.servo[b] = sv;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.plant[(size_t)b * 8 + i] = st[i];
    r.step[b] += n;
}

// the delayed form of race_command_plant_observe_kernel (lpvmpc_race_init_actuated with an estimator): the plant gets the actuator
// stage's output, the observer the commanded (servo, motor) (stateEstimator.py:785 subscribes to `ecu`); a frozen vehicle advances
// neither plant, actuator nor observer
__global__ void __launch_bounds__(64) race_command_plant_observe_act_kernel(RaceDev r, PlantCfg pc, const double *__restrict__ gains,
                                                                            double *__restrict__ obs, ObsParams op, ActDev a) {
    __shared__ double G[kObsGainWords];
    obs_stage_gains(G, gains);
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
    const int k0 = a.k[b], La = a.La[b], Ld = a.Ld[b];
    double sv = a.servo[b];
    for (int k = 0; k < n; ++k) {
        asm volatile("" ::: "memory");               // as in race_command_plant_observe_kernel
        double ua, ud;
        act_stage(a, b, k0 + k, La, Ld, motor, servo, sv, ua, ud);
        plant_step(pc, st, ua, ud);
        obs_substep(G, op, vid, os, st, servo, motor);
    }
    a.k[b] = k0 + n; a.servo[b] = sv;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.plant[(size_t)b * 8 + i] = st[i];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
    double *v = r.estv + (size_t)b * 8;
    v[0] = os[3]; v[1] = os[4]; v[2] = os[0]; v[3] = os[1]; v[4] = 0.0; v[5] = 0.0; v[6] = os[5]; v[7] = os[2];
    r.step[b] += n;
}

#define LPVMPC_GRID(n) dim3(((n) + 63) / 64), dim3(64)
hipError_t launch_plant_actuated(int B, double *plant, const double *u, PlantCfg pc, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(plant_actuated_kernel, LPVMPC_GRID(B), 0, s, B, plant, u, pc, a);
    return hipGetLastError();
}
hipError_t launch_cl_measure_act(const DevCfg *dcfg, int B, const double *plant, const double *cmd, double hw, double slack, int q9_swap,
                                 double *local_state, double *u_old, int sd, hipStream_t s) {
    hipLaunchKernelGGL(cl_measure_act_kernel, LPVMPC_GRID(B), 0, s, dcfg, B, plant, cmd, hw, slack, q9_swap, local_state, u_old, sd);
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_measure_act(const DevCfg *dcfg, int B, int N, const double *uPred, double *cmd, double *plant, PlantCfg pc,
                                               double hw, double slack, int q9_swap, double *local_next, double *u_old, int sd,
                                               const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_measure_act_kernel, LPVMPC_GRID(B), 0, s, dcfg, B, N, uPred, cmd, plant, pc, hw, slack, q9_swap,
                       local_next, u_old, sd, a);
    return hipGetLastError();
}

hipError_t launch_cl_observe_measure_act(const DevCfg *dcfg, int B, const double *obs, const double *cmd, double hw, double slack, int q9_swap,
                                         double *local_state, double *u_old, int sd, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_act_kernel, LPVMPC_GRID(B), 0, s, dcfg, B, 1, (const double *)nullptr, const_cast<double *>(cmd),
                       (double *)nullptr, PlantCfg{}, hw, slack, q9_swap, local_state, u_old, (const double *)nullptr, const_cast<double *>(obs),
                       ObsParams{}, 0, sd, ActDev{});
    return hipGetLastError();
}
hipError_t launch_cl_command_plant_observe_act(const DevCfg *dcfg, int B, int N, const double *uPred, double *cmd, double *plant, PlantCfg pc,
                                              double hw, double slack, int q9_swap, double *local_next, double *u_old, int sd,
                                              const double *gains, double *obs, const ObsParams &op, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(cl_command_plant_observe_act_kernel, LPVMPC_GRID(B), 0, s, dcfg, B, N, uPred, cmd, plant, pc, hw, slack, q9_swap,
                       local_next, u_old, gains, obs, op, 1, sd, a);
    return hipGetLastError();
}

hipError_t launch_race_measure_act(const DevCfg *ccfg, const RaceDev &r, int seed_tick, int sd, hipStream_t s) {
    hipLaunchKernelGGL(race_measure_act_kernel, LPVMPC_GRID(r.B), 0, s, ccfg, r, seed_tick, sd);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_act(const RaceDev &r, PlantCfg pc, const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_act_kernel, LPVMPC_GRID(r.B), 0, s, r, pc, a);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe_act(const RaceDev &r, PlantCfg pc, const double *gains, double *obs, const ObsParams &op,
                                                const ActDev &a, hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_observe_act_kernel, LPVMPC_GRID(r.B), 0, s, r, pc, gains, obs, op, a);
    return hipGetLastError();
}

}  // namespace lpvmpc
