// observer_device.hpp -- device functions of the gain-scheduled LPV state estimator and its simulated sensors, shared by
// observer.hip, race.hip and the estimator kernels of fleet_kernels.hpp: the noise generator, one observer step, sensors + one
// observer step after a plant step, the LDS staging of the gain words and the controller's measurement from the estimate.  Every
// includer is compiled with -ffp-contract=off, so every includer computes the same words.
#pragma once
#include "lpvmpc_device.hpp"
#include "track_geometry.hpp"

namespace lpvmpc {

constexpr int kObsGainWords = 2 * (kObsTable + 12);    // [L_ls][lim_ls][L_hs][lim_hs]: the head of lpvmpc_observer_config

// ---- counter-based noise (documented in lpvmpc.h) -----------------------------------------------------------------------
__device__ inline unsigned long long obs_mix(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ inline double obs_gauss(unsigned long long seed, long long vid, long long step, int ch) {
    const unsigned long long g = 0x9E3779B97F4A7C15ull;
    const unsigned long long key = obs_mix(obs_mix(seed + g * ((unsigned long long)vid + 1ull)) ^ (8ull * (unsigned long long)step + (unsigned long long)ch));
    const double u1 = (double)((obs_mix(key + g) >> 11) + 1ull) * 0x1.0p-53;
    const double u2 = (double)(obs_mix(key + 2ull * g) >> 11) * 0x1.0p-53;
    return sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
}
// clip(std * g, +-std * n_bound); a channel whose std is 0 draws nothing and adds 0
__device__ inline double obs_noise(const ObsParams &p, long long vid, long long step, int ch) {
    const double sd = p.std[ch];
    if (sd == 0.0) return 0.0;
    const double n = sd * obs_gauss(p.seed, vid, step, ch), lim = sd * p.n_bound;
    return n > lim ? lim : (n < -lim ? -lim : n);
}

// ---- per-vehicle estimator (lpvmpc_set_observer_vehicles) -----------------------------------------------------------------
// The binding's device tables (ObsVehDev, lpvmpc_device.hpp).  ObsVeh<false> is empty: the forms without the flag take and read
// nothing.  ObsGainsArg is the `gains` argument of the fused observe kernels: the gain words' pointer, with the flag the binding's
// tables next to it (ObsVehGains)
template <bool kObsVeh> struct ObsVeh {};
template <> struct ObsVeh<true> : ObsVehDev {};
template <bool kObsVeh> struct ObsGainsArg { using type = const double *__restrict__; };
template <> struct ObsGainsArg<true> { using type = ObsVehGains; };
__device__ inline const double *obs_gain_words(const double *g) { return g; }
__device__ inline const double *obs_gain_words(const ObsVehGains &a) { return a.g; }
__device__ inline ObsVeh<false> obs_veh(const double *) { return {}; }
__device__ inline ObsVeh<true> obs_veh(const ObsVehGains &a) { ObsVeh<true> v; static_cast<ObsVehDev &>(v) = a; return v; }

// ---- one GS_LPV_Est step (EST:349-398) ------------------------------------------------------------------------------------
// G: the gain words (LDS); x [6] in/out; y [5]; t = k dt.  L [30], A [36], Bm [12] receive the step's matrices.
// kObsVeh: the seven model words are vehicle b's row of ov.rows and the polytope's gain words come from ov.L (global memory);
// limits, the polytope switch and the weights stay G's.  Every value is formed by the same operations in the same order.
template <bool kObsVeh = false>
__device__ inline void obs_step(const double *G, double x[6], const double y[5], double servo, double motor, double k, double dt,
                                double L[30], double A[36], double Bm[12], ObsVeh<kObsVeh> ov = {}, int b = 0) {
    const double t = k * dt;
    const bool run = t > 0.02;
    const double vx = run ? x[0] : y[0], vy = run ? x[1] : 0.0, th = run ? x[5] : y[4];
    const double steer = servo;
    // Continuous_AB_Comp (EST:402-436): the observer's own constants
    double lf = 0.125, lr = 0.125, m = 1.98, I = 0.03, Cf = 60, Cr = 60, mu = 0.05;
    if constexpr (kObsVeh) {
        const double *r = ov.rows + b;
        const size_t n = ov.B;
        lf = r[0]; lr = r[n]; m = r[2 * n]; I = r[3 * n]; Cf = r[4 * n]; Cr = r[5 * n]; mu = r[6 * n];
    }
    double ss, cs, sth, cth;
    sincos(steer, &ss, &cs);
    sincos(th, &sth, &cth);
    Bm[0] = -(ss * Cf) / m; Bm[1] = 1.0;
    Bm[2] = (cs * Cf) / m;  Bm[3] = 0.0;
    Bm[4] = (lf * Cf * cs) / I; Bm[5] = 0.0;
#pragma unroll
    for (int i = 6; i < 12; ++i) Bm[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 36; ++i) A[i] = 0.0;
    A[0] = -mu;
    A[1] = (ss * Cf) / (m * vx);
    A[2] = (ss * Cf * lf) / (m * vx) + vy;
    A[7] = -(Cr + Cf * cs) / (m * vx);
    A[8] = -(lf * Cf * cs - lr * Cr) / (m * vx) - vx;
    A[13] = -(lf * Cf * cs - lr * Cr) / (I * vx);
    A[14] = -(lf * lf * Cf * cs + lr * lr * Cr) / (I * vx);
    A[18] = cth; A[19] = -sth;
    A[24] = sth; A[25] = cth;
    A[32] = 1.0;
    // L_Gain_Comp (EST:439-492): polytope choice, unclamped vertex weights, blend
    const bool hs = vx > G[kObsTable + 1];
    const double *Lg = hs ? G + kObsTable + 12 : G;
    const double *lim = Lg + kObsTable;
    size_t gs = 1;                                                      // words between a polytope's consecutive gain words
    if constexpr (kObsVeh) { gs = ov.B; Lg = ov.L + (hs ? (size_t)kObsTable * gs : 0) + b; }
    const double Mvx = (lim[1] - vx) / (lim[1] - lim[0]);
    const double Mvy = (lim[3] - vy) / (lim[3] - lim[2]);
    const double Mst = (lim[7] - steer) / (lim[7] - lim[6]);
    const double Mth = (lim[11] - th) / (lim[11] - lim[10]);
    double w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const double a = (i & 8) ? 1 - Mvx : Mvx, b = (i & 4) ? 1 - Mvy : Mvy, c = (i & 2) ? 1 - Mst : Mst, d = (i & 1) ? 1 - Mth : Mth;
        w[i] = a * b * c * d;
    }
#pragma unroll
    for (int e = 0; e < 30; ++e) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += w[i] * Lg[(e * 16 + i) * gs];
        L[e] = s;
    }
    // x+ = x + (dt (A + L C) x + dt B u - dt L y), C = rows {0, 2, 3, 4, 5} of I6 (EST:248-252)
    double xn[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double M0 = A[r * 6 + 0] + L[r * 5 + 0], M1 = A[r * 6 + 1], M2 = A[r * 6 + 2] + L[r * 5 + 1],
                     M3 = A[r * 6 + 3] + L[r * 5 + 2], M4 = A[r * 6 + 4] + L[r * 5 + 3], M5 = A[r * 6 + 5] + L[r * 5 + 4];
        const double Mx = M0 * x[0] + M1 * x[1] + M2 * x[2] + M3 * x[3] + M4 * x[4] + M5 * x[5];
        const double Bu = Bm[r * 2 + 0] * servo + Bm[r * 2 + 1] * motor;
        const double Ly = L[r * 5 + 0] * y[0] + L[r * 5 + 1] * y[1] + L[r * 5 + 2] * y[2] + L[r * 5 + 3] * y[3] + L[r * 5 + 4] * y[4];
        xn[r] = x[r] + (dt * Mx + dt * Bu - dt * Ly);
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) x[r] = xn[r];
}

// ---- sensors + one observer step after a plant step ------------------------------------------------------------------------
// os [kObsStride]: see ObsSlot; st = plant state just advanced.  kObsVeh, ov, b: as obs_step.
template <bool kObsVeh = false>
__device__ inline void obs_substep(const double *G, const ObsParams &p, long long vid, double *os, const double st[8], double servo,
                                   double motor, ObsVeh<kObsVeh> ov = {}, int b = 0) {
    const double k = os[OBS_K] + 1.0;
    os[OBS_K] = k;
    const long long step = (long long)k;
    const double imu_yaw = st[6] + obs_noise(p, vid, step, 0);
    const double imu_w = st[7] + obs_noise(p, vid, step, 1);
    const double gx = st[0] + obs_noise(p, vid, step, 2), gy = st[1] + obs_noise(p, vid, step, 3);
    // SIM:296-305: publish when the counter exceeds thUpdate, then restart it
    const bool pub = os[OBS_GPS_CNT] > p.th_update;
    os[OBS_GPS_CNT] = pub ? 0.0 : os[OBS_GPS_CNT] + 1.0;
    os[OBS_GPS_X] = pub ? gx : os[OBS_GPS_X];
    os[OBS_GPS_Y] = pub ? gy : os[OBS_GPS_Y];
    // EST:733-741: a changed reading is taken; more than 40 unchanged readings in a row read 0 (v_prev becomes v either way)
    const double v = sqrt(st[2] * st[2] + st[3] * st[3]) + obs_noise(p, vid, step, 4);
    const bool changed = v != os[OBS_ENC_PREV];
    os[OBS_ENC_CNT] = changed ? 0.0 : os[OBS_ENC_CNT] + 1.0;
    os[OBS_ENC_MEAS] = changed ? v : (os[OBS_ENC_CNT] > 40.0 ? 0.0 : os[OBS_ENC_MEAS]);
    os[OBS_ENC_PREV] = v;
    // EST:330-333: the start-up measurement
    const bool run = k * p.dt > 0.02;
    double y[5];
    y[0] = run ? os[OBS_ENC_MEAS] : os[0];
    y[1] = imu_w; y[2] = os[OBS_GPS_X]; y[3] = os[OBS_GPS_Y];
    y[4] = run ? imu_yaw : st[6];
    double L[30], A[36], Bm[12];
    obs_step<kObsVeh>(G, os, y, servo, motor, k, p.dt, L, A, Bm, ov, b);
#pragma unroll
    for (int i = 0; i < 5; ++i) os[OBS_Y + i] = y[i];
}

__device__ inline void obs_stage_gains(double *lds, const double *__restrict__ g) {
    for (int i = threadIdx.x; i < kObsGainWords; i += blockDim.x) lds[i] = g[i];
    __syncthreads();
}

// controller measurement from the estimate (the estimator path's cl_measure_kernel): [max(vx, 0.01), vy, psiDot] and the map's
// local frame of (x, y, yaw) with quirk Q9 as in cl_local
__device__ inline void obs_local_state(const double *T, int rows, double hw, double slack, int q9_swap, const double *e, double *ls) {
    double s, ey, epsi; int inside;
    local_position(T, rows, hw, slack, e[3], e[4], e[5], s, ey, epsi, inside);
    ls[0] = e[0] < 0.01 ? 0.01 : e[0]; ls[1] = e[1]; ls[2] = e[2];
    ls[3] = q9_swap ? ey : epsi; ls[4] = s; ls[5] = q9_swap ? epsi : ey;
}
__device__ __forceinline__ void obs_local_state(const DevCfg &c, double hw, double slack, int q9_swap, const double *e, double *ls) {
    obs_local_state(c.track, c.track_rows, hw, slack, q9_swap, e, ls);
}

}  // namespace lpvmpc
