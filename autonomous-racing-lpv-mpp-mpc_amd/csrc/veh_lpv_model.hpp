// veh_lpv_model.hpp -- the per-vehicle LPV model, once: the model row, the stage blocks and the roll-out / linearisation bodies of the
// kernels of veh_lpv_eval.hip (per-vehicle model rows, the handle's track) and track_lpv_eval.hip (per-vehicle model rows and
// tracks).  The bodies that read the track are templates over the curvature source `trk`: OwnTrack, the configuration's own table, or
// the vehicle's view of the track palette (const TrackView &, track_view.hpp).  OwnTrack is an empty tag and not a second reference
// to the configuration: with `c` passed twice ctrl_abc_veh_kernel and plan_abc_veh_kernel lost one instruction each (777 -> 776,
// 730 -> 729: the load of c.dt moved in front of the curvature loop), with the tag every kernel keeps its code.  Each of the two
// objects instantiates one form only, and each compiles to the code it had with a copy of its own (tools/isa_equal.py).
//
// The stage blocks and roll-outs restate those of lpv_eval.hip with a VehModel `v` in the place of the configuration's vehicle
// words: every value is formed by the same operations in the same order (the includers are compiled with -ffp-contract=off like
// lpv_eval.o), so a row equal to the handle's words gives the per-handle kernels' bits -- tests/test_gpu_model_params.py holds the
// files together, word for word, on every route.  lpv_eval.hip does not include this header and keeps its own text: with the stage
// functions in a header that it instantiates too (vehicle type as a template argument), LLVM compiled five of the six kernels of
// lpv_eval.o to other code, and tests/test_model_params_host.py pins its source.  The three plant_step* functions of
// track_geometry.hpp are out of scope for the same reason: their comment records the same measurement.
#pragma once
#include "lpvmpc_device.hpp"

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

// the curvature source of a body: the configuration's own table (OwnTrack: nothing to pass), or the vehicle's view of the track palette
struct OwnTrack {};
__device__ __forceinline__ double stage_curvature(const DevCfg &c, OwnTrack, double s) { return track_curvature(c, s); }
template <class Trk> __device__ __forceinline__ double stage_curvature(const DevCfg &, const Trk &trk, double s) { return track_curvature(trk, s); }

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

// controller roll-out of instance b, CTRL:166-258.  cf: the tyre stiffness of BOTH axles (the reference passes Cf_new for both,
// CTRL:203-218): the call's cf_new, or the vehicle's own Cf in the per-vehicle form
template <class Trk>
__device__ __forceinline__ void ctrl_lpv_body(const DevCfg &c, const Trk &trk, const VehModel &v, double cf, int b, const double *x0,
                                     const double *u_prev, const double *vel_ref,
                                     const double *curv_ref, int lap, double *states, double *AB) {
    const int N = c.N;
    double st[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) st[r] = x0[(size_t)b * 6 + r];
    for (int i = 0; i < N; ++i) {
        const double vy = st[1], epsi = st[3], s = st[4], ey = st[5];
        const double cur = (lap == 0) ? stage_curvature(c, trk, s) : curv_ref[(size_t)b * N + i];
        const double vx = vel_ref[(size_t)b * (N + 1) + i];                 // quirk Q5: vx from vel_ref
        const double u0 = u_prev[((size_t)b * N + i) * 2 + 0], u1 = u_prev[((size_t)b * N + i) * 2 + 1];
        double ab[6][8];
        ctrl_stage(c, v, cf, cf, vx, vy, epsi, ey, cur, u0, ab);
        double nx[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) acc += ab[r][a] * st[a];
            nx[r] = acc + (ab[r][6] * u0 + ab[r][7] * u1);
        }
        if (AB) {
            double *o = AB + ((size_t)b * N + i) * 48;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int a = 0; a < 8; ++a) o[r * 8 + a] = ab[r][a];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            st[r] = nx[r];
            if (states) states[((size_t)b * N + i) * 6 + r] = nx[r];
        }
    }
}

// the state-independent part of controller stage t = b * N + i (ctrl_lpv_pre_kernel, lpv_eval.hip); cf as in ctrl_lpv_body
__device__ inline void ctrl_lpv_pre_body(const DevCfg &c, const VehModel &v, double cf, int b, int i, int t, const double *u_prev,
                                         const double *vel_ref, double *AB) {
    const int N = c.N;
    const double vx = vel_ref[(size_t)b * (N + 1) + i], delta = u_prev[(size_t)t * 2];
    const double Cf = cf, Cr = cf, m = v.m, I = v.Iz, lf = v.lf, lr = v.lr, dt = c.dt;
    double sd, cd;
    sincos(delta, &sd, &cd);
    const double a12 = (sd * Cf) / (m * vx);
    const double p13 = (sd * Cf * lf) / (m * vx);                  // a13 = p13 + vy
    const double a22 = -(Cr + Cf * cd) / (m * vx);
    const double a23 = -(lf * Cf * cd - lr * Cr) / (m * vx) - vx;
    const double a32 = -(lf * Cf * cd - lr * Cr) / (I * vx);
    const double a33 = -(lf * lf * Cf * cd + lr * lr * Cr) / (I * vx);
    const double b11 = -(sd * Cf) / m, b21 = (cd * Cf) / m, b31 = (lf * Cf * cd) / I;
    double ab[6][8];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int a = 0; a < 8; ++a) ab[r][a] = 0.0;
    ab[0][0] = 1.0 + dt * (-v.mu); ab[0][1] = dt * a12; ab[0][2] = p13;
    ab[1][1] = 1.0 + dt * a22;     ab[1][2] = dt * a23;
    ab[2][1] = dt * a32;           ab[2][2] = 1.0 + dt * a33;
    ab[3][2] = dt * 1.0; ab[3][3] = 1.0;
    ab[4][4] = 1.0;
    ab[5][5] = 1.0;
    ab[0][6] = dt * b11; ab[0][7] = dt * 1.0;
    ab[1][6] = dt * b21;
    ab[2][6] = dt * b31;
    double *o = AB + (size_t)t * 48;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int a = 0; a < 8; ++a) o[r * 8 + a] = ab[r][a];
}

// controller seed-mode linearisation of stage t, CTRL:732-809 (vx from the trajectory, curvature from the map)
template <class Trk>
__device__ __forceinline__ void ctrl_abc_body(const DevCfg &c, const Trk &trk, const VehModel &v, int t, const double *xlast,
                                     const double *delta, double *AB) {
    const double *x = xlast + (size_t)t * 6;
    const double cur = stage_curvature(c, trk, x[4]);
    double ab[6][8];
    ctrl_stage(c, v, v.Cf, v.Cr, x[0], x[1], x[3], x[5], cur, delta[t], ab);
    double *o = AB + (size_t)t * 48;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int a = 0; a < 8; ++a) o[r * 8 + a] = ab[r][a];
}

// planner roll-out of instance b, PLAN:242-320
template <class Trk>
__device__ __forceinline__ void plan_lpv_body(const DevCfg &c, const Trk &trk, const VehModel &v, int b, const double *x0, const double *u_prev,
                                     const double *SS, double *states, double *AB) {
    const int N = c.N;
    double st[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) st[r] = x0[(size_t)b * 5 + r];
    for (int i = 0; i < N; ++i) {
        const double cur = stage_curvature(c, trk, SS[(size_t)b * (N + 1) + i]);
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
template <class Trk>
__device__ __forceinline__ void plan_abc_body(const DevCfg &c, const Trk &trk, const VehModel &v, int t, const double *xlast,
                                     const double *delta, double *AB) {
    const double *x = xlast + (size_t)t * 6;
    const double cur = stage_curvature(c, trk, x[5]);
    double ab[5][7];
    plan_stage(c, v, x[0], x[1], x[3], x[4], cur, delta[t], ab);
    double *o = AB + (size_t)t * 35;
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int a = 0; a < 7; ++a) o[r * 7 + a] = ab[r][a];
}

}  // namespace lpvmpc
