// track_race.hip -- the bound forms of the race's and the hand-off's kernels that read the track (include/lpvmpc.h, "Per-vehicle
// tracks"): every vehicle measures, counts its laps, starts its planner, integrates its planned path and is recorded on its own entry
// of the track palette, with that entry's length, half width and slack.
//   race_measure_trk_kernel      race_measure_kernel<true> of fleet_kernels.hpp: the lap-event rules take the vehicle's own lap length
//                                L (HalfTrack at 3L/4, the event at s <= L/4, the racing rule s >= L - L/10)
//   race_plan_start_trk_kernel   race_plan_start_kernel of race.hip (plan_first_one on the vehicle's track)
//   plan_pose_trk_kernel         plan_pose_kernel of handoff.hip (curvature and centre-line pose from the vehicle's track)
//   race_record_trk_kernel       race_record_kernel of record.hip (the ground-truth track frame)
// Each restates its original with the vehicle's track view where the original passes the configuration: the same statements in the
// same order, compiled as race.o, handoff.o and record.o are, so that a palette entry equal to a handle's table gives that handle's
// words.  race_command_plant* and tt_measure_kernel read no track and have no form here.  Their own object, so that race.o,
// actuator.o, handoff.o and record.o keep the code they have alone.
//
// One source for each pair was tried, the body as a forced-inline function template over the track source (the configuration, or the
// binding) that both kernels call, and measured on the device code (tools/isa_equal.py; DESIGN.md, "One source, one form per object").
// None of the four pairs kept its instruction streams, so all four stay restated (instructions before -> after):
//   race_measure          race_measure_kernel<false> 3254 -> 3365 (race.o), <true> 3279 -> 3390 (actuator.o), race_measure_trk_kernel
//                         3218 -> 3311
//   race_plan_start       plan_first_one, which both objects call as a function, was inlined instead: race_plan_start_kernel
//                         370 -> 2215, race_plan_start_trk_kernel 388 -> 2174
//   plan_pose             plan_pose_kernel 1901 -> 1901 (handoff.o) and plan_pose_trk_kernel 1894 -> 1894, both with the entry's address
//                         arithmetic scheduled elsewhere and a loop's compare inverted
//   race_record           race_record_kernel 2048 -> 2046 (record.o), race_record_trk_kernel 2024 -> 2022 (other registers), with the
//                         recorder's argument by reference or by value
#include "record.hpp"
#include "track_view.hpp"

namespace lpvmpc {

// measurement, lap logic and this tick's controller masks on the vehicle's own track
__global__ void __launch_bounds__(64) race_measure_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, RaceDev r, int seed_tick, int sd) {
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
    double hw, slack;
    const TrackView tv = track_view(trk, b, hw, slack);
    const double L = tv.T[(tv.rows - 1) * 6 + 3] + tv.T[(tv.rows - 1) * 6 + 4];      // the vehicle's own lap length
    double *ls = r.local + (size_t)b * 6;
    bool event = false;
    int k = 0;
    if (ph == 0) {                                                          // CMAIN:186-190
        cl_local(tv, hw, slack, r.q9, p, ls);
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

// first launch of a tick: the planner ticks of the racing vehicles, the first one from the state measured on the vehicle's track
__global__ void __launch_bounds__(64) race_plan_start_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, RaceDev r) {
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
                double hw, slack;
                const TrackView tv = track_view(trk, b, hw, slack);
                plan_first_one(c, tv, m, hw, slack, r.q9, 0.2, x0, r.q_xlast + (size_t)b * Np * 6, r.q_delta + (size_t)b * Np);
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

// PMAIN:201-224 on the vehicle's track
__global__ void __launch_bounds__(64) plan_pose_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, int B, const double *__restrict__ xPred,
                                                       double *__restrict__ SS, double *__restrict__ pose, double *__restrict__ sig,
                                                       const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (active && !active[b])) return;
    const int N = c.N;
    const TrackView tv = track_view(trk, b);
    const double *xp = xPred + (size_t)b * (N + 1) * 5;
    double *ss = SS + (size_t)b * (N + 1), *sg = sig + (size_t)b * 5 * N;
    double X = pose[b * 3 + 0], Y = pose[b * 3 + 1], Th = pose[b * 3 + 2];
    double s = ss[0], s1 = 0.0;
    for (int j = 0; j < N; ++j) {
        const double vx = xp[j * 5 + 0], vy = xp[j * 5 + 1], wz = xp[j * 5 + 2], ey = xp[j * 5 + 3], epsi = xp[j * 5 + 4];
        const double yaw = Th + epsi;                                   // Xref[j], Yref[j], Thetaref[j] belong to stage j
        sg[0 * N + j] = X - ey * sin(yaw);
        sg[1 * N + j] = Y + ey * cos(yaw);
        sg[2 * N + j] = yaw;
        sg[3 * N + j] = vx;
        sg[4 * N + j] = wz / vx;
        const double cv = track_curvature(tv, s);
        s = s + ((vx * cos(epsi) - vy * sin(epsi)) / (1 - ey * cv)) * c.dt;
        ss[j + 1] = s;
        global_position(tv, s, 0.0, X, Y, Th);
        if (j == 0) { s1 = s; pose[b * 3 + 0] = X; pose[b * 3 + 1] = Y; pose[b * 3 + 2] = Th; }   // Xlast = Xref[1] ...
    }
    ss[0] = s1;                                                         // SS[0] = SS[1]  (PMAIN:216)
}

__global__ void __launch_bounds__(64) race_record_trk_kernel(TrackDev trk, RecDev r, int t, int slot) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= r.B) return;
    const size_t B = r.B;
    const double *p = r.plant + (size_t)b * 8, *ls = r.local + (size_t)b * 6;
    const int ph = r.phase[b], lap = r.lap[b], src = r.src[b], it = r.iters[b], st = r.status[b];
    const int planned = r.m_plan[b] != 0;
    const int pit = planned ? r.q_iters[b] : -1, pst = planned ? r.q_status[b] : -1;
    // the node's References row: [0 0 0 1] on ticks measured by the lap-0 branch (the event tick included: phase 1, rk 0 after it),
    // else the point Body_Frame_Errors used and vel_ref[0]
    const bool lap0_branch = ph == 0 || (ph == 1 && r.rk[b] == 0);
    double ref[4] = {0.0, 0.0, 0.0, 1.0};
    if (!lap0_branch) {
        ref[0] = r.ref0[b * 3 + 0]; ref[1] = r.ref0[b * 3 + 1]; ref[2] = r.ref0[b * 3 + 2];
        ref[3] = r.t_vel[(size_t)b * (r.N + 1)];
    }
    double ts, tey, tepsi;
    int inside;
    double hw, slack;
    const TrackView tv = track_view(trk, b, hw, slack);
    local_position(tv, hw, slack, p[0], p[1], p[6], ts, tey, tepsi, inside);     // the ground-truth plant's track frame
    if (slot >= 0) {
        double *f = r.rec_f + (size_t)slot * LPVMPC_REC_F64 * B + b;
#pragma unroll
        for (int i = 0; i < 8; ++i) f[(LPVMPC_REC_PLANT + i) * B] = p[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) f[(LPVMPC_REC_LOCAL + i) * B] = ls[i];
        f[(LPVMPC_REC_CMD + 0) * B] = r.cmd[b * 2 + 0]; f[(LPVMPC_REC_CMD + 1) * B] = r.cmd[b * 2 + 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[(LPVMPC_REC_REF + i) * B] = ref[i];
        f[(LPVMPC_REC_TRACK + 0) * B] = ts; f[(LPVMPC_REC_TRACK + 1) * B] = tey; f[(LPVMPC_REC_TRACK + 2) * B] = tepsi;
        if (r.obs) {
            const double *os = r.obs + (size_t)b * kObsStride;                  // [vx vy psiDot x y yaw ...]
#pragma unroll
            for (int i = 0; i < 6; ++i) f[(LPVMPC_REC_EST + i) * B] = os[i];
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) f[(LPVMPC_REC_EST + i) * B] = __builtin_nan("");
        }
        int32_t *g = r.rec_i + (size_t)slot * LPVMPC_REC_I32 * B + b;
        g[LPVMPC_REC_PHASE * B] = ph; g[LPVMPC_REC_LAP * B] = lap; g[LPVMPC_REC_SRC * B] = src;
        g[LPVMPC_REC_ITERS * B] = it; g[LPVMPC_REC_STATUS * B] = st;
        g[LPVMPC_REC_PLAN_ITERS * B] = pit; g[LPVMPC_REC_PLAN_STATUS * B] = pst; g[LPVMPC_REC_INSIDE * B] = inside;
    }
    // per-lap statistics
    if (r.prev_phase[b] < 2 && ph >= 2) r.end_tick[b] = t;
    r.prev_phase[b] = ph;
    if (src < 0 || lap < 0 || lap > r.laps) return;        // frozen, lost and finishing ticks do not count
    double *sf = r.stat_f + ((size_t)b * (r.laps + 1) + lap) * LPVMPC_LAPSTAT_F64;
    int32_t *si = r.stat_i + ((size_t)b * (r.laps + 1) + lap) * LPVMPC_LAPSTAT_I32;
    // ey / epsi of the measurement: slots 5 / 3, except on a lap-0-branch tick with q9_swap (quirk Q9 stores them in 3 / 5)
    const bool swapped = r.q9 && lap0_branch;
    const double ev = ls[0] - ref[3], ey = swapped ? ls[3] : ls[5], epsi = swapped ? ls[5] : ls[3];
    sf[LPVMPC_LAPSTAT_SSE_V] = sf[LPVMPC_LAPSTAT_SSE_V] + ev * ev;
    sf[LPVMPC_LAPSTAT_SSE_EY] = sf[LPVMPC_LAPSTAT_SSE_EY] + ey * ey;
    sf[LPVMPC_LAPSTAT_SSE_EPSI] = sf[LPVMPC_LAPSTAT_SSE_EPSI] + epsi * epsi;
    if (fabs(ey) > sf[LPVMPC_LAPSTAT_MAX_EY]) sf[LPVMPC_LAPSTAT_MAX_EY] = fabs(ey);
    sf[LPVMPC_LAPSTAT_SUM_VX] = sf[LPVMPC_LAPSTAT_SUM_VX] + ls[0];
    if (fabs(tey) > sf[LPVMPC_LAPSTAT_MAX_EY_TRACK]) sf[LPVMPC_LAPSTAT_MAX_EY_TRACK] = fabs(tey);
    si[LPVMPC_LAPSTAT_TICKS] += 1;
    si[LPVMPC_LAPSTAT_CTRL_ITERS] += it;
    if (it > si[LPVMPC_LAPSTAT_CTRL_ITERS_MAX]) si[LPVMPC_LAPSTAT_CTRL_ITERS_MAX] = it;
    si[LPVMPC_LAPSTAT_CTRL_NOT_SOLVED] += st != LPVMPC_SOLVED;
    if (planned) {
        si[LPVMPC_LAPSTAT_PLAN_TICKS] += 1;
        si[LPVMPC_LAPSTAT_PLAN_ITERS] += pit;
        if (pit > si[LPVMPC_LAPSTAT_PLAN_ITERS_MAX]) si[LPVMPC_LAPSTAT_PLAN_ITERS_MAX] = pit;
        si[LPVMPC_LAPSTAT_PLAN_NOT_SOLVED] += pst != LPVMPC_SOLVED;
    }
    si[LPVMPC_LAPSTAT_OFF_TRACK] += inside == 0;
}

hipError_t launch_race_plan_start_trk(const DevCfg *pcfg, const TrackDev &trk, const RaceDev &r, hipStream_t s) {
    hipLaunchKernelGGL(race_plan_start_trk_kernel, LPVMPC_GRID(r.B), 0, s, pcfg, trk, r);
    return hipGetLastError();
}
hipError_t launch_race_measure_trk(const RaceMeasureArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(race_measure_trk_kernel, LPVMPC_GRID(a.r.B), 0, s, a.ccfg, *a.trk, a.r, a.seed_tick, a.sd);
    return hipGetLastError();
}
hipError_t launch_plan_pose_trk(const DevCfg *dcfg, const TrackDev &trk, int B, const double *xPred, double *SS, double *pose, double *sig,
                                hipStream_t s, const int32_t *active) {
    hipLaunchKernelGGL(plan_pose_trk_kernel, LPVMPC_GRID(B), 0, s, dcfg, trk, B, xPred, SS, pose, sig, active);
    return hipGetLastError();
}
hipError_t launch_race_record_trk(const TrackDev &trk, const RecDev &r, int t, int slot, hipStream_t s) {
    hipLaunchKernelGGL(race_record_trk_kernel, LPVMPC_GRID(r.B), 0, s, trk, r, t, slot);
    return hipGetLastError();
}

}  // namespace lpvmpc
