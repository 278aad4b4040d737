// track_lpv_eval.hip -- the bound forms of the LPV kernels that read the track (include/lpvmpc.h, "Per-vehicle tracks"): vehicle b
// looks its curvature up in its own entry of the handle's track palette (lpvmpc_set_tracks; TrackDev, track_view.hpp) instead of the
// table of the handle's configuration.  dt and N stay the handle's.
//
// They are per-vehicle-model forms all: the stage blocks and roll-outs below restate those of veh_lpv_eval.hip, with the vehicle's
// track view `tv` where they pass the configuration to track_curvature -- every value is formed by the same operations in the same
// order (this object is compiled with -ffp-contract=off like lpv_eval.o and veh_lpv_eval.o), so a palette entry equal to the
// handle's table gives their bits.  A handle without bound model rows runs them on the binding's table of the handle's own vehicle
// words.  The controller roll-out has its two-launch form only (every caller of the library wants [A | B]): ctrl_lpv_pre_kernel, or
// its per-vehicle form, reads no track and is launched as it is -- it is where the call's cf_new or the row's Cf enters -- and
// ctrl_lpv_roll_trk_kernel restates ctrl_lpv_roll_kernel of lpv_eval.hip, which reads no vehicle word.
// Restated and not shared for the reason
// veh_lpv_eval.hip gives: the per-handle and per-vehicle kernels must not move.
#include "lpvmpc_device.hpp"
#include "track_view.hpp"

namespace lpvmpc {

// one row of the model table [kModelWords][B] (parameter-major, vehicle-minor: a wavefront's loads of one word coalesce)
struct VehModel {
    double lf, lr, m, Iz, Cf, Cr, mu;
};
__device__ inline VehModel load_model(const double *__restrict__ p, int B, int b) {
    VehModel v;
    v.lf = p[(size_t)0 * B + b]; v.lr = p[(size_t)1 * B + b]; v.m = p[(size_t)2 * B + b]; v.Iz = p[(size_t)3 * B + b];
    v.Cf = p[(size_t)4 * B + b]; v.Cr = p[(size_t)5 * B + b]; v.mu = p[(size_t)6 * B + b];
    return v;
}

// continuous-time entries shared by both models (CTRL:203-218 == PLAN:275-286)
struct Tyre {
    double a12, a13, a22, a23, a32, a33, b11, b21, b31;
};

__device__ inline Tyre tyre_terms(const VehModel &c, double Cf, double Cr, double vx, double vy, double delta) {
    Tyre t;
    double sd, cd;
    sincos(delta, &sd, &cd);           // one argument reduction for both (the roll-out is a serial chain of these calls)
    const double m = c.m, I = c.Iz, lf = c.lf, lr = c.lr;
    t.a12 = (sd * Cf) / (m * vx);
    t.a13 = (sd * Cf * lf) / (m * vx) + vy;
    t.a22 = -(Cr + Cf * cd) / (m * vx);
    t.a23 = -(lf * Cf * cd - lr * Cr) / (m * vx) - vx;
    t.a32 = -(lf * Cf * cd - lr * Cr) / (I * vx);
    t.a33 = -(lf * lf * Cf * cd + lr * lr * Cr) / (I * vx);
    t.b11 = -(sd * Cf) / m;
    t.b21 = (cd * Cf) / m;
    t.b31 = (lf * Cf * cd) / I;
    return t;
}

// controller stage: fills ab[6][8] = [I + dt*Ac | dt*Bc]   (CTRL:220-246)
__device__ inline void ctrl_stage(const DevCfg &c, const VehModel &v, double Cf, double Cr, double vx, double vy, double epsi,
                                  double ey, double cur, double delta, double ab[6][8]) {
    const Tyre t = tyre_terms(v, Cf, Cr, vx, vy, delta);
    const double dt = c.dt;
    double se, ce;
    sincos(epsi, &se, &ce);
    const double den = 1.0 - ey * cur;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int a = 0; a < 8; ++a) ab[r][a] = 0.0;
    ab[0][0] = 1.0 + dt * (-v.mu); ab[0][1] = dt * t.a12; ab[0][2] = dt * t.a13;
    ab[1][1] = 1.0 + dt * t.a22;   ab[1][2] = dt * t.a23;
    ab[2][1] = dt * t.a32;         ab[2][2] = 1.0 + dt * t.a33;
    ab[3][0] = dt * ((1.0 / den) * (-ce * cur)); ab[3][1] = dt * ((1.0 / den) * (se * cur)); ab[3][2] = dt * 1.0; ab[3][3] = 1.0;
    ab[4][0] = dt * (ce / den);    ab[4][1] = dt * (se / den);  ab[4][4] = 1.0;
    ab[5][0] = dt * se;            ab[5][1] = dt * ce;          ab[5][5] = 1.0;
    ab[0][6] = dt * t.b11; ab[0][7] = dt * 1.0;
    ab[1][6] = dt * t.b21;
    ab[2][6] = dt * t.b31;
}

// planner stage: fills ab[5][7]   (PLAN:288-308), states [vx vy wz ey epsi]
__device__ inline void plan_stage(const DevCfg &c, const VehModel &v, double vx, double vy, double ey, double epsi, double cur,
                                  double delta, double ab[5][7]) {
    const Tyre t = tyre_terms(v, v.Cf, v.Cr, vx, vy, delta);
    const double dt = c.dt;
    const double A1 = 1.0 / (1.0 - ey * cur);
    const double A2 = sin(epsi);
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int a = 0; a < 7; ++a) ab[r][a] = 0.0;
    ab[0][0] = 1.0 + dt * (-v.mu); ab[0][1] = dt * t.a12; ab[0][2] = dt * t.a13;
    ab[1][1] = 1.0 + dt * t.a22;   ab[1][2] = dt * t.a23;
    ab[2][1] = dt * t.a32;         ab[2][2] = 1.0 + dt * t.a33;
    ab[3][1] = dt * 1.0;           ab[3][3] = 1.0;  ab[3][4] = dt * vx;
    ab[4][0] = dt * (-A1 * cur);   ab[4][1] = dt * (A1 * A2 * cur); ab[4][2] = dt * 1.0; ab[4][4] = 1.0;
    ab[0][5] = dt * t.b11; ab[0][6] = dt * 1.0;
    ab[1][5] = dt * t.b21;
    ab[2][5] = dt * t.b31;
}

// controller seed-mode linearisation of stage t, CTRL:732-809 (vx from the trajectory, curvature from the map)
__device__ inline void ctrl_abc_body(const DevCfg &c, const TrackView &tv, const VehModel &v, int t, const double *xlast,
                                     const double *delta, double *AB) {
    const double *x = xlast + (size_t)t * 6;
    const double cur = track_curvature(tv, x[4]);
    double ab[6][8];
    ctrl_stage(c, v, v.Cf, v.Cr, x[0], x[1], x[3], x[5], cur, delta[t], ab);
    double *o = AB + (size_t)t * 48;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int a = 0; a < 8; ++a) o[r * 8 + a] = ab[r][a];
}

// planner roll-out of instance b, PLAN:242-320
__device__ inline void plan_lpv_body(const DevCfg &c, const TrackView &tv, const VehModel &v, int b, const double *x0, const double *u_prev,
                                     const double *SS, double *states, double *AB) {
    const int N = c.N;
    double st[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) st[r] = x0[(size_t)b * 5 + r];
    for (int i = 0; i < N; ++i) {
        const double cur = track_curvature(tv, SS[(size_t)b * (N + 1) + i]);
        const double u0 = u_prev[((size_t)b * N + i) * 2 + 0], u1 = u_prev[((size_t)b * N + i) * 2 + 1];
        double ab[5][7];
        plan_stage(c, v, st[0], st[1], st[3], st[4], cur, u0, ab);
        double nx[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int a = 0; a < 5; ++a) acc += ab[r][a] * st[a];
            nx[r] = acc + (ab[r][5] * u0 + ab[r][6] * u1);
        }
        if (AB) {
            double *o = AB + ((size_t)b * N + i) * 35;
#pragma unroll
            for (int r = 0; r < 5; ++r)
#pragma unroll
                for (int a = 0; a < 7; ++a) o[r * 7 + a] = ab[r][a];
        }
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            st[r] = nx[r];
            if (states) states[((size_t)b * N + i) * 5 + r] = nx[r];
        }
    }
}

// planner seed-mode linearisation of stage t, PLAN:519-591; xlast columns [vx vy wz ey epsi s]
__device__ inline void plan_abc_body(const DevCfg &c, const TrackView &tv, const VehModel &v, int t, const double *xlast,
                                     const double *delta, double *AB) {
    const double *x = xlast + (size_t)t * 6;
    const double cur = track_curvature(tv, x[5]);
    double ab[5][7];
    plan_stage(c, v, x[0], x[1], x[3], x[4], cur, delta[t], ab);
    double *o = AB + (size_t)t * 35;
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int a = 0; a < 7; ++a) o[r * 7 + a] = ab[r][a];
}

// ctrl_lpv_roll_kernel (lpv_eval.hip) on the vehicle's track: the state-dependent entries of the tiles that ctrl_lpv_pre_kernel (or
// its per-vehicle form) wrote, and the roll-out
__global__ void __launch_bounds__(64) ctrl_lpv_roll_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, int B, const double *__restrict__ x0,
                                                               const double *__restrict__ u_prev, const double *__restrict__ curv_ref,
                                                               int lap, double *__restrict__ states, double *__restrict__ AB,
                                                               const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (active && !active[b])) return;
    const TrackView tv = track_view(trk, b);
    const int N = c.N;
    const double dt = c.dt;
    double st[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) st[r] = x0[(size_t)b * 6 + r];
    for (int i = 0; i < N; ++i) {
        double *o = AB + ((size_t)b * N + i) * 48;
        const double a00 = o[0], a01 = o[1], p13 = o[2], a11 = o[9], a12_ = o[10], a21 = o[17], a22_ = o[18];
        const double b06 = o[6], b07 = o[7], b16 = o[14], b26 = o[22];
        const double vy = st[1], epsi = st[3], s = st[4], ey = st[5];
        const double cur = (lap == 0) ? track_curvature(tv, s) : curv_ref[(size_t)b * N + i];
        const double u0 = u_prev[((size_t)b * N + i) * 2 + 0], u1 = u_prev[((size_t)b * N + i) * 2 + 1];
        double se, ce;
        sincos(epsi, &se, &ce);
        const double den = 1.0 - ey * cur;
        const double a02 = dt * (p13 + vy);
        const double a30 = dt * ((1.0 / den) * (-ce * cur)), a31 = dt * ((1.0 / den) * (se * cur)), a32 = dt * 1.0;
        const double a40 = dt * (ce / den), a41 = dt * (se / den);
        const double a50 = dt * se, a51 = dt * ce;
        double nx[6];
        nx[0] = ((a00 * st[0] + a01 * st[1]) + a02 * st[2]) + (b06 * u0 + b07 * u1);
        nx[1] = (a11 * st[1] + a12_ * st[2]) + (b16 * u0 + 0.0 * u1);
        nx[2] = (a21 * st[1] + a22_ * st[2]) + (b26 * u0 + 0.0 * u1);
        nx[3] = (((a30 * st[0] + a31 * st[1]) + a32 * st[2]) + 1.0 * st[3]) + (0.0 * u0 + 0.0 * u1);
        nx[4] = ((a40 * st[0] + a41 * st[1]) + 1.0 * st[4]) + (0.0 * u0 + 0.0 * u1);
        nx[5] = ((a50 * st[0] + a51 * st[1]) + 1.0 * st[5]) + (0.0 * u0 + 0.0 * u1);
        o[2] = a02;
        o[24] = a30; o[25] = a31;
        o[32] = a40; o[33] = a41;
        o[40] = a50; o[41] = a51;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            st[r] = nx[r];
            if (states) states[((size_t)b * N + i) * 6 + r] = nx[r];
        }
    }
}

__global__ void __launch_bounds__(64) ctrl_abc_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, const double *__restrict__ model, int B,
                                                          const double *__restrict__ xlast, const double *__restrict__ delta,
                                                          double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = c.N;
    if (t >= B * N || (active && !active[t / N])) return;
    ctrl_abc_body(c, track_view(trk, t / N), load_model(model, B, t / N), t, xlast, delta, AB);
}

__global__ void __launch_bounds__(64) plan_lpv_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, const double *__restrict__ model, int B,
                                                          const double *__restrict__ x0, const double *__restrict__ u_prev,
                                                          const double *__restrict__ SS, double *__restrict__ states,
                                                          double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (active && !active[b])) return;
    plan_lpv_body(c, track_view(trk, b), load_model(model, B, b), b, x0, u_prev, SS, states, AB);
}

__global__ void __launch_bounds__(64) plan_abc_trk_kernel(const DevCfg *__restrict__ cp, TrackDev trk, const double *__restrict__ model, int B,
                                                          const double *__restrict__ xlast, const double *__restrict__ delta,
                                                          double *__restrict__ AB, const int32_t *__restrict__ active) {
    const DevCfg &c = *cp;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = c.N;
    if (t >= B * N || (active && !active[t / N])) return;
    plan_abc_body(c, track_view(trk, t / N), load_model(model, B, t / N), t, xlast, delta, AB);
}

void launch_ctrl_lpv_roll_trk(const DevCfg *dcfg, const TrackDev &trk, int B, const double *x0, const double *u_prev, const double *curv_ref,
                              int lap, double *states, double *AB, hipStream_t stream, const int32_t *active) {
    hipLaunchKernelGGL(ctrl_lpv_roll_trk_kernel, LPVMPC_GRID(B), 0, stream, dcfg, trk, B, x0, u_prev, curv_ref, lap, states, AB, active);
}
void launch_plan_lpv_trk(const DevCfg *dcfg, const TrackDev &trk, const double *model, int B, const double *x0, const double *u_prev,
                         const double *SS, double *states, double *AB, hipStream_t stream, const int32_t *active) {
    hipLaunchKernelGGL(plan_lpv_trk_kernel, LPVMPC_GRID(B), 0, stream, dcfg, trk, model, B, x0, u_prev, SS, states, AB, active);
}
void launch_abc_trk(int kind, const DevCfg *dcfg, const TrackDev &trk, const double *model, int B, int N, const double *xlast,
                    const double *delta, double *AB, hipStream_t stream, const int32_t *active) {
    if (kind == 0) hipLaunchKernelGGL(ctrl_abc_trk_kernel, LPVMPC_GRID(B * N), 0, stream, dcfg, trk, model, B, xlast, delta, AB, active);
    else hipLaunchKernelGGL(plan_abc_trk_kernel, LPVMPC_GRID(B * N), 0, stream, dcfg, trk, model, B, xlast, delta, AB, active);
}

}  // namespace lpvmpc
