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
// The measurement and command / plant kernels are in fleet_kernels.hpp (this file launches their plain forms).
#include "lpvmpc_device.hpp"
#include "observer_device.hpp"
#include "track_geometry.hpp"
#include "fleet_kernels.hpp"

namespace lpvmpc {

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

hipError_t launch_race_plan_start(const DevCfg *pcfg, const RaceDev &r, hipStream_t s) {
    hipLaunchKernelGGL(race_plan_start_kernel, LPVMPC_GRID(r.B), 0, s, pcfg, r);
    return hipGetLastError();
}
hipError_t launch_race_measure(const RaceMeasureArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(race_measure_kernel<false>, LPVMPC_GRID(a.r.B), 0, s, a.ccfg, a.r, a.seed_tick, 0);
    return hipGetLastError();
}
hipError_t launch_race_command_plant(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_kernel<false>, LPVMPC_GRID(a.r.B), 0, s, a.r, a.pc, ActDev{});
    return hipGetLastError();
}
hipError_t launch_race_command_plant_observe(const RaceStepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(race_command_plant_observe_kernel<false>, LPVMPC_GRID(a.r.B), 0, s, a.r, a.pc, a.gains.g, a.obs, a.op, ActDev{});
    return hipGetLastError();
}

}  // namespace lpvmpc
