// race.hip -- per-tick glue of the race engine (lpvmpc_race_*): a fleet runs the reference's whole experiment,
// lap 0 under the path-following controller, the lap event, then planner + trajectory-tracking controller until it
// has driven its laps.  Every vehicle has its own phase, so one tick of the fleet mixes lap-0 vehicles, vehicles on their
// event tick and racing vehicles, each at its own planner phase.  One lane per vehicle, as closed_loop.hip / handoff.hip,
// whose per-vehicle recipes (track_geometry.hpp) these kernels share.
//
// Replaces, per vehicle and with nothing on the host between ticks:
//   controllerMain.py:176-190,198-283   both measurement branches, HalfTrack, the two lap-event rules, the lap counter
//   controllerMain.py:286-298,326-336   u_old of the controller of the vehicle's lap; on the event tick the trajectory-tracking
//                                       controller takes the path controller's uPred and the lap-0 references (ones / zeros)
//   plannerMain.py:129,137-141          the planner runs from the tick after the vehicle's lap event, first from the measured state
//   controllerMain.py:381-386           command from the controller of the vehicle's lap, then the simulator steps
//
// The masks written here select the instances of this tick's masked launches (LPV, solve, hand-off: SolveArgs::active).
//
// With the estimator in the loop (lpvmpc_race_init_observed) every measurement -- both branches, both lap-event rules and the
// planner's first state -- reads RaceDev::meas = the estimate view instead of the plant (CMAIN:179-180 and PMAIN:141 read
// pos_info), and race_command_plant_observe_kernel runs sensors + one observer step after each plant step.
#include "lpvmpc_device.hpp"
#include "observer_device.hpp"
#include "track_geometry.hpp"

namespace lpvmpc {

__device__ inline bool plant_finite(const double *p) {
    bool fin = true;
    for (int i = 0; i < 8; ++i) fin = fin && __builtin_isfinite(p[i]);
    return fin;
}

// first launch of a tick: which racing vehicles run a planner tick before this controller tick (planner ticks
// 0 .. floor(2k/3) precede racing tick k), and their initial state -- measured from the plant on the vehicle's first planner
// tick (plus the seed trajectory the ABC linearisation needs), Planner.xPred[1] on the later ones (replaces the cascade's
// strided device copy).  c is the planner's configuration.  "Measured" reads r.meas: the plant, or the estimate.
__global__ void __launch_bounds__(64) race_plan_start_kernel(const DevCfg *__restrict__ cp, RaceDev r) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= r.B) return;
    int first = 0, cont = 0;
    const double *p = r.plant + (size_t)b * 8, *m = r.meas + (size_t)b * 8;
    if (r.phase[b] == 1 && plant_finite(p) && plant_finite(m)) {
        const int k = r.rk[b], done = r.plan_done[b];
        if (done <= (2 * k) / 3) {
            const int Np = c.N;
            double *x0 = r.q_x0 + (size_t)b * 5;
            if (done == 0) {
                plan_first_one(c, m, r.hw, r.slack, r.q9, 0.2, x0, r.q_xlast + (size_t)b * Np * 6, r.q_delta + (size_t)b * Np);
                first = 1;
            } else {
                const double *xp = r.q_xPred + (size_t)b * (Np + 1) * 5 + 5;
                for (int i = 0; i < 5; ++i) x0[i] = xp[i];
                cont = 1;
            }
            r.plan_done[b] = done + 1;
        }
    }
    r.m_pfirst[b] = first; r.m_pcont[b] = cont; r.m_plan[b] = first | cont;
}

// Copied in actuator.hip as race_measure_act_kernel (the delayed race), which differs only in the u_old write: change both
// (tests/test_actuator_kernel_copies.py compares them).
// measurement (from r.meas), lap logic and this tick's controller masks.  c is the controllers' configuration (path and TT share
// N, dt, track).  A vehicle entering the tick with a non-finite plant or measurement source is lost.
// seed_tick: the race's first 9 ticks (first_it < 10, CMAIN:310-320) solve the path controller on the seed trajectories.
__global__ void __launch_bounds__(64) race_measure_kernel(const DevCfg *__restrict__ cp, RaceDev r, int seed_tick) {
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
    uo[b * 2 + 0] = r.cmd[b * 2 + 0]; uo[b * 2 + 1] = r.cmd[b * 2 + 1];
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

// last launch of a tick: the solve's report, the command of the vehicle's controller and its simulator steps.  This kernel
// and race_command_plant_observe_kernel have delayed copies in actuator.hip (the plant steps through act_stage): change both
__global__ void __launch_bounds__(64) race_command_plant_kernel(RaceDev r, PlantCfg pc) {
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
    for (int k = 0; k < n; ++k) plant_step(pc, st, motor, servo);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.plant[(size_t)b * 8 + i] = st[i];
    r.step[b] += n;
}

// race_command_plant_kernel with the estimator in the loop: per plant step, plant -> sensors -> observer (obs_substep, the schedule
// of cl_command_plant_observe_kernel), then the estimate view that the next tick's measurements read.  A frozen vehicle (nstep 0)
// advances neither the plant nor its observer, so its noise keys (vid, step) depend on its own steps only.
__global__ void __launch_bounds__(64) race_command_plant_observe_kernel(RaceDev r, PlantCfg pc, const double *__restrict__ gains,
                                                                        double *__restrict__ obs, ObsParams op) {
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
    for (int k = 0; k < n; ++k) {
        // compiler-only barrier: without it the gain words' LDS loads (read-only after the staging barrier) are hoisted out of
        // the loop for both polytopes, 1968 registers' worth, and spill to scratch (6.7 KB per lane)
        asm volatile("" ::: "memory");
        plant_step(pc, st, motor, servo);
        obs_substep(G, op, vid, os, st, servo, motor);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) r.plant[(size_t)b * 8 + i] = st[i];
#pragma unroll
    for (int i = 0; i < kObsStride; ++i) obs[(size_t)b * kObsStride + i] = os[i];
    double *v = r.estv + (size_t)b * 8;
    v[0] = os[3]; v[1] = os[4]; v[2] = os[0]; v[3] = os[1]; v[4] = 0.0; v[5] = 0.0; v[6] = os[5]; v[7] = os[2];
    r.step[b] += n;
}

#define LPVMPC_GRID(n) dim3(((n) + 63) / 64), dim3(64)
hipError_t launch_race_plan_start(const DevCfg *pcfg, const RaceDev &r, hipStream_t s) {
    hipLaunchKernelGGL(race_plan_start_kernel, LPVMPC_GRID(r.B), 0, s, pcfg, r);
    return hipGetLastError();
}
hipError_t launch_race_measure(const DevCfg *ccfg, const RaceDev &r, int seed_tick, hipStream_t s) {
    hipLaunchKernelGGL(race_measure_kernel, LPVMPC_GRID(r.B), 0, s, ccfg, r, seed_tick);
    return hipGetLastError();
}
hipError_t launch_race_command_plant(const RaceDev &r, PlantCfg pc, hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_kernel, LPVMPC_GRID(r.B), 0, s, r, pc);
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe(const RaceDev &r, PlantCfg pc, const double *gains, double *obs, const ObsParams &op,
                                            hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_observe_kernel, LPVMPC_GRID(r.B), 0, s, r, pc, gains, obs, op);
    return hipGetLastError();
}

}  // namespace lpvmpc
