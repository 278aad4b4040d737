// record.hip -- the race recorder (lpvmpc_race_record): the data the reference's controller node logs (controllerMain.py:
// ALL_LOCAL_DATA, GLOBAL_DATA, References CMAIN:194-195,217-218,411-412) and the per-lap tracking statistics it declares
// (RMSE_ve / RMSE_ye / RMSE_thetae, CMAIN:101-106,115,419), kept on the device so that a race enqueued with
// lpvmpc_race_tick(n) needs nothing on the host between ticks.  One lane per vehicle; launched after the tick's command / plant
// kernel, while recording is on.  It reads race state only and writes the recorder's buffers only.
//
// Its own translation unit (compiled with -ffp-contract=off, as race.o): adding a kernel to race.hip or fleet_kernels.hpp could
// change the code of the kernels there.  The sums below are s = s + x * x in tick order without contraction, so a replay of the
// stride-1 trace in tick order (telemetry.py) reproduces every word.
#include "record.hpp"
#include "track_geometry.hpp"

namespace lpvmpc {

__global__ void __launch_bounds__(64) race_record_kernel(const DevCfg *__restrict__ cp, RecDev r, int t, int slot) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= r.B) return;
    const DevCfg &c = *cp;
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
    local_position(c, r.hw, r.slack, p[0], p[1], p[6], ts, tey, tepsi, inside);     // the ground-truth plant's track frame
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

hipError_t launch_race_record(const DevCfg *ccfg, const RecDev &r, int t, int slot, hipStream_t s) {
    hipLaunchKernelGGL(race_record_kernel, dim3((r.B + 63) / 64), dim3(64), 0, s, ccfg, r, t, slot);
    return hipGetLastError();
}

}  // namespace lpvmpc
