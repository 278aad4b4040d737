// track_geometry.hpp -- device functions shared by closed_loop.hip and handoff.hip: track coordinate transforms
// and the plant model, one call per vehicle.
//   Map.getLocalPosition     Utilities/trackInitialization.py:283-383 (+ computeAngle :393-411)
//   Map.getGlobalPosition    Utilities/trackInitialization.py:205-262
//   wrap / sign              Utilities/trackInitialization.py:413-431
//   Simulator.f              vehicleSimulator.py:164-199
#pragma once
#include "lpvmpc_device.hpp"

namespace lpvmpc {

constexpr double kPi = 3.14159265358979323846;

__device__ inline double wrap_pi(double a) {          // TRACK:414-422
    if (a < -kPi) return 2 * kPi + a;
    if (a > kPi) return a - 2 * kPi;
    return a;
}
__device__ inline double sgn1(double a) { return a >= 0 ? 1.0 : -1.0; }   // TRACK:425-431 (sign(0) = +1)
// numpy.unwrap([a, b])[1]
__device__ inline double unwrap2(double a, double b) {
    const double dd = b - a;
    double ddmod = fmod(dd + kPi, 2 * kPi);
    if (ddmod < 0) ddmod += 2 * kPi;
    ddmod -= kPi;
    if (ddmod == -kPi && dd > 0) ddmod = kPi;
    double corr = ddmod - dd;
    if (fabs(dd) < kPi) corr = 0.0;
    return b + corr;
}
// computeAngle(point1, origin, point2), TRACK:393-411
__device__ inline double compute_angle(double p1x, double p1y, double ox, double oy, double p2x, double p2y) {
    const double v1x = p1x - ox, v1y = p1y - oy, v2x = p2x - ox, v2y = p2y - oy;
    return atan2(v1x * v2y - v1y * v2x, v1x * v2x + v1y * v2y);
}
__device__ inline double norm2(double x, double y) { return sqrt(x * x + y * y); }

// The functions that read the track are written once, on a table T [rows][6] of PointAndTangent rows; the forms on the configuration's
// own table (DevCfg::track) follow each, the forms on a palette entry are in track_view.hpp.  All of them forward, but for
// plan_first_one (see there).
//
// A kernel body shared by a form on the handle's own track and a form on per-vehicle tracks is a template over its track source `src`,
// the configuration or the binding (TrackDev, track_view.hpp), and looks the vehicle's track up with track_view(src, b, hw, slack)
// where the bound form does.  The configuration is its own view, and hw and slack stay the caller's.
__device__ __forceinline__ const DevCfg &track_view(const DevCfg &c, int, double &, double &) { return c; }
__device__ __forceinline__ const DevCfg &track_view(const DevCfg &c, int) { return c; }

// Map.getLocalPosition: (x, y, psi) -> (s, ey, epsi, inside); 10000 sentinels when off the track (TRACK:376-379)
__device__ __forceinline__ void local_position(const double *T, int rows, double hw, double slack, double x, double y, double psi,
                                               double &s, double &ey, double &epsi, int &inside) {
    int done = 0;
    s = ey = epsi = 0.0;
    for (int i = 0; i < rows && !done; ++i) {
        const int ip = i > 0 ? i - 1 : rows - 1;                       // PointAndTangent[i - 1] wraps to the last row
        const double xf = T[i * 6 + 0], yf = T[i * 6 + 1], xs = T[ip * 6 + 0], ys = T[ip * 6 + 1];
        if (T[i * 6 + 5] == 0.0) {                                      // straight segment
            epsi = unwrap2(T[ip * 6 + 2], psi) - T[ip * 6 + 2];
            if (norm2(xs - x, ys - y) == 0) { s = T[i * 6 + 3]; ey = 0; done = 1; }
            else if (norm2(xf - x, yf - y) == 0) { s = T[i * 6 + 3] + T[i * 6 + 4]; ey = 0; done = 1; }
            else if (fabs(compute_angle(x, y, xs, ys, xf, yf)) <= kPi / 2 && fabs(compute_angle(x, y, xf, yf, xs, ys)) <= kPi / 2) {
                const double n1 = norm2(x - xs, y - ys);
                const double ang = compute_angle(xf, yf, xs, ys, x, y);
                s = n1 * cos(ang) + T[i * 6 + 3];
                ey = n1 * sin(ang);
                if (fabs(ey) <= hw + slack) done = 1;
            }
        } else {
            const double r = 1 / T[i * 6 + 5];
            const double d = r >= 0 ? 1.0 : -1.0;
            const double ang = T[ip * 6 + 2];
            const double cx = xs + fabs(r) * cos(ang + d * kPi / 2), cy = ys + fabs(r) * sin(ang + d * kPi / 2);
            if (norm2(xs - x, ys - y) == 0) { ey = 0; epsi = unwrap2(ang, psi) - ang; s = T[i * 6 + 3]; done = 1; }
            else if (norm2(xf - x, yf - y) == 0) {
                s = T[i * 6 + 3] + T[i * 6 + 4]; ey = 0; epsi = unwrap2(T[i * 6 + 2], psi) - T[i * 6 + 2]; done = 1;
            } else {
                const double arc1 = T[i * 6 + 4] * T[i * 6 + 5];
                const double arc2 = compute_angle(xs, ys, cx, cy, x, y);
                const double s1 = arc1 > 0 ? 1.0 : (arc1 < 0 ? -1.0 : 0.0), s2 = arc2 > 0 ? 1.0 : (arc2 < 0 ? -1.0 : 0.0);
                if (s1 == s2 && fabs(arc1) >= fabs(arc2)) {
                    s = fabs(arc2) * fabs(r) + T[i * 6 + 3];
                    ey = -d * (norm2(x - cx, y - cy) - fabs(r));
                    epsi = unwrap2(ang + arc2, psi) - (ang + arc2);
                    if (fabs(ey) <= hw + slack) done = 1;
                }
            }
        }
    }
    inside = done;
    if (!done) { s = 10000; ey = 10000; epsi = 10000; }
}
__device__ __forceinline__ void local_position(const DevCfg &c, double hw, double slack, double x, double y, double psi,
                                               double &s, double &ey, double &epsi, int &inside) {
    local_position(c.track, c.track_rows, hw, slack, x, y, psi, s, ey, epsi, inside);
}

// Map.getGlobalPosition: (s, ey) -> (x, y, theta).  Where the reference fails (no segment contains s) NaNs are returned.
__device__ inline void global_position(const double *T, int rows, double s, double ey, double &x, double &y, double &th) {
    const double L = T[(rows - 1) * 6 + 3] + T[(rows - 1) * 6 + 4];
    s = wrap_track_s(s, L);      // NaN beyond kMaxWrapLaps laps / non-finite s: no segment below, NaNs returned
    int i = -1;
    for (int k = 0; k < rows; ++k) if (s >= T[k * 6 + 3] && s < T[k * 6 + 3] + T[k * 6 + 4]) { i = k; break; }
    if (i < 0) { x = y = th = __builtin_nan(""); return; }
    const int ip = i > 0 ? i - 1 : rows - 1;
    if (T[i * 6 + 5] == 0.0) {
        const double xf = T[i * 6 + 0], yf = T[i * 6 + 1], xs = T[ip * 6 + 0], ys = T[ip * 6 + 1], psi = T[i * 6 + 2];
        const double dL = T[i * 6 + 4], rL = s - T[i * 6 + 3];
        x = (1 - rL / dL) * xs + rL / dL * xf + ey * cos(psi + kPi / 2);
        y = (1 - rL / dL) * ys + rL / dL * yf + ey * sin(psi + kPi / 2);
        th = psi;
    } else {
        const double r = 1 / T[i * 6 + 5], ang = T[ip * 6 + 2];
        const double d = r >= 0 ? 1.0 : -1.0;
        const double cx = T[ip * 6 + 0] + fabs(r) * cos(ang + d * kPi / 2), cy = T[ip * 6 + 1] + fabs(r) * sin(ang + d * kPi / 2);
        const double span = (s - T[i * 6 + 3]) / (kPi * fabs(r)) * kPi;
        const double an = wrap_pi(d * kPi / 2 + ang);
        const double a0 = -(kPi - fabs(an)) * sgn1(an);
        x = cx + (fabs(r) - d * ey) * cos(a0 + d * span);
        y = cy + (fabs(r) - d * ey) * sin(a0 + d * span);
        th = ang + d * span;
    }
}
__device__ __forceinline__ void global_position(const DevCfg &c, double s, double ey, double &x, double &y, double &th) {
    global_position(c.track, c.track_rows, s, ey, x, y, th);
}

// Simulator.f: st = [x y vx vy ax ay yaw psiDot], u = [a, delta]
__device__ inline void plant_step(const PlantCfg &p, double st[8], double ua, double ud) {
    const double x = st[0], y = st[1], vx = st[2], vy = st[3], ax = st[4], ay = st[5], yaw = st[6], w = st[7];
    double aF = 0.0, aR = 0.0;
    if (fabs(vx) > 0.2) {
        aF = ud - atan((vy + p.lf * w) / fabs(vx));
        aR = atan((-vy + p.lr * w) / fabs(vx));
    }
    const double FyF = 60 * aF, FyR = 60 * aR;
    st[0] = x + p.dt * (cos(yaw) * vx - sin(yaw) * vy);
    st[1] = y + p.dt * (sin(yaw) * vx + cos(yaw) * vy);
    st[2] = fabs(vx + p.dt * (ax + w * vy));
    st[3] = vy + p.dt * (ay - w * vx);
    st[4] = ua - p.mu * vx - FyF / p.m * sin(ud);
    st[5] = 1.0 / p.m * (FyF * cos(ud) + FyR);
    st[6] = yaw + p.dt * w;
    st[7] = w + p.dt * (1.0 / p.Iz * (p.lf * FyF * cos(ud) - p.lr * FyR));
}

// Simulator.f with one vehicle's parameter row q = [lf lr m Iz Cf Cr mu] (lpvmpc_*_vehicles): plant_step's expressions with the tyre
// stiffnesses Cf, Cr where Simulator.f has 60, so that the nominal row (Cf = Cr = 60) gives plant_step's bits
__device__ inline void plant_step_row(const double q[kPlantWords], double dt, double st[8], double ua, double ud) {
    const double lf = q[0], lr = q[1], m = q[2], Iz = q[3], Cf = q[4], Cr = q[5], mu = q[6];
    const double x = st[0], y = st[1], vx = st[2], vy = st[3], ax = st[4], ay = st[5], yaw = st[6], w = st[7];
    double aF = 0.0, aR = 0.0;
    if (fabs(vx) > 0.2) {
        aF = ud - atan((vy + lf * w) / fabs(vx));
        aR = atan((-vy + lr * w) / fabs(vx));
    }
    const double FyF = Cf * aF, FyR = Cr * aR;
    st[0] = x + dt * (cos(yaw) * vx - sin(yaw) * vy);
    st[1] = y + dt * (sin(yaw) * vx + cos(yaw) * vy);
    st[2] = fabs(vx + dt * (ax + w * vy));
    st[3] = vy + dt * (ay - w * vx);
    st[4] = ua - mu * vx - FyF / m * sin(ud);
    st[5] = 1.0 / m * (FyF * cos(ud) + FyR);
    st[6] = yaw + dt * w;
    st[7] = w + dt * (1.0 / Iz * (lf * FyF * cos(ud) - lr * FyR));
}

// one tyre's lateral force at slip angle ang for the tyre row ty = [kind B C c_f]: kind 0 the linear tyre C_lin * ang, kind 1
// Simulator.pacejka (vehicleSimulator.py:202-205), D sin(C atan(B ang)) with D = c_f m g / 2 associated as the reference writes it
__device__ inline double tyre_force(const double ty[kTyreWords], double m, double C_lin, double ang) {
    if (ty[0] == 0.0) return C_lin * ang;
    const double D = ty[3] * m * 9.81 / 2;
    return D * sin(ty[2] * atan(ty[1] * ang));
}

// plant_step_row with the vehicle's tyre row on both axles (lpvmpc_*_tyres): its expressions, written out again because sharing them
// with plant_step_row through a helper changes the per-vehicle forms' code, with tyre_force where it has Cf * aF, Cr * aR -- a kind 0
// row gives plant_step_row's bits
__device__ inline void plant_step_tyre_row(const double q[kPlantWords], const double ty[kTyreWords], double dt, double st[8], double ua,
                                           double ud) {
    const double lf = q[0], lr = q[1], m = q[2], Iz = q[3], Cf = q[4], Cr = q[5], mu = q[6];
    const double x = st[0], y = st[1], vx = st[2], vy = st[3], ax = st[4], ay = st[5], yaw = st[6], w = st[7];
    double aF = 0.0, aR = 0.0;
    if (fabs(vx) > 0.2) {
        aF = ud - atan((vy + lf * w) / fabs(vx));
        aR = atan((-vy + lr * w) / fabs(vx));
    }
    const double FyF = tyre_force(ty, m, Cf, aF), FyR = tyre_force(ty, m, Cr, aR);
    st[0] = x + dt * (cos(yaw) * vx - sin(yaw) * vy);
    st[1] = y + dt * (sin(yaw) * vx + cos(yaw) * vy);
    st[2] = fabs(vx + dt * (ax + w * vy));
    st[3] = vy + dt * (ay - w * vx);
    st[4] = ua - mu * vx - FyF / m * sin(ud);
    st[5] = 1.0 / m * (FyF * cos(ud) + FyR);
    st[6] = yaw + dt * w;
    st[7] = w + dt * (1.0 / Iz * (lf * FyF * cos(ud) - lr * FyR));
}

// one simulator step of vehicle b in a fleet kernel: the fleet's PlantCfg (plain and delayed forms), or the vehicle's row of the
// table (per-vehicle forms) and of the tyre table (tyre forms), read at every step -- a cached, coalesced load instead of seven or
// eleven more registers held across the loop
__device__ __forceinline__ void plant_step_at(const PlantCfg &p, int, double st[8], double ua, double ud) { plant_step(p, st, ua, ud); }
__device__ __forceinline__ void plant_step_at(const VehPlantCfg &p, int b, double st[8], double ua, double ud) {
    double q[kPlantWords];
#pragma unroll
    for (int i = 0; i < kPlantWords; ++i) q[i] = p.p[(size_t)i * p.B + b];
    plant_step_row(q, p.dt, st, ua, ud);
}
__device__ __forceinline__ void plant_step_at(const TyrePlantCfg &p, int b, double st[8], double ua, double ud) {
    double q[kPlantWords], ty[kTyreWords];
#pragma unroll
    for (int i = 0; i < kPlantWords; ++i) q[i] = p.p[(size_t)i * p.B + b];
#pragma unroll
    for (int i = 0; i < kTyreWords; ++i) ty[i] = p.t[(size_t)i * p.B + b];
    plant_step_tyre_row(q, ty, p.dt, st, ua, ud);
}

// Actuator stage of one simulator step (vehicleSimulator.py:67-76) for vehicle b at its plant step kk: the command (motor, servo)
// enters the two FIFOs and the plant receives the entries La / Ld steps old -- 0 while kk < L, the FIFOs start filled with zeros;
// L = 0 is the command itself.  With lowLevelDyn the servo filter sv runs on the delayed steering and is what the plant receives.
// The slot of step kk - L is read before step kk's command overwrites it, so L = kActRing needs no extra slot.
__device__ inline void act_stage(const ActDev &a, int b, int kk, int La, int Ld, double motor, double servo, double &sv, double &ua, double &ud) {
    constexpr int m = kActRing - 1;
    double *ra = a.ring + b, *rd = a.ring + (size_t)kActRing * a.B + b;
    ua = La == 0 ? motor : (kk >= La ? ra[(size_t)((kk - La) & m) * a.B] : 0.0);
    ud = Ld == 0 ? servo : (kk >= Ld ? rd[(size_t)((kk - Ld) & m) * a.B] : 0.0);
    ra[(size_t)(kk & m) * a.B] = motor;
    rd[(size_t)(kk & m) * a.B] = servo;
    if (a.lld) { sv = a.c1 * sv + a.c * ud; ud = sv; }        // (1 - T/Tf) * servo_inp + (T/Tf) * df_his.pop(0)
}

// CMAIN:289-298 for a controller with steeringDelay sd: OldSteering (1 + sd entries) and OldAccelera (1 entry) append the last
// command and drop their oldest entry.  u [2 + sd] = [OldSteering[0], OldAccelera[0], OldSteering[1 .. sd]] (include/lpvmpc.h, u_old);
// sd = 0 leaves u = [servo, motor], the write of the fleets without a steering delay
__device__ inline void uold_push(double *u, int sd, double servo, double motor) {
    if (sd > 0) {
        u[0] = u[2];
        for (int j = 2; j < 1 + sd; ++j) u[j] = u[j + 1];
        u[1 + sd] = servo;
    } else u[0] = servo;
    u[1] = motor;
}

// a plant state (or the estimate view in its layout) whose 8 words are finite
__device__ inline bool plant_finite(const double *p) {
    bool fin = true;
    for (int i = 0; i < 8; ++i) fin = fin && __builtin_isfinite(p[i]);
    return fin;
}

// ---- per-vehicle measurement recipes shared by the fleet engines (closed_loop.hip, handoff.hip, race.hip) ----
// lap-0 measurement (CMAIN:183-188): local state from the plant's ground truth, vx clamped at 0.01; q9_swap = SURVEY quirk Q9
__device__ __forceinline__ void cl_local(const double *T, int rows, double hw, double slack, int q9_swap, const double *p, double *ls) {
    double s, ey, epsi; int inside;
    local_position(T, rows, hw, slack, p[0], p[1], p[6], s, ey, epsi, inside);
    ls[0] = p[2] < 0.01 ? 0.01 : p[2]; ls[1] = p[3]; ls[2] = p[7];
    ls[3] = q9_swap ? ey : epsi; ls[4] = s; ls[5] = q9_swap ? epsi : ey;
}
__device__ __forceinline__ void cl_local(const DevCfg &c, double hw, double slack, int q9_swap, const double *p, double *ls) {
    cl_local(c.track, c.track_rows, hw, slack, q9_swap, p, ls);
}

// LapNumber >= 1 measurement (CMAIN:198-248): yaw unwound by the lap counter, Body_Frame_Errors against the first sample of
// the reference window (ref0 = x, y, yaw; cv0 = its curvature), s dead-reckoned from SS
__device__ __forceinline__ void tt_local(const DevCfg &c, const double *p, int lap, const double *ref0, double cv0, double SS, double *ls) {
    const double vx = p[2] < 0.01 ? 0.01 : p[2], vy = p[3];
    const double psi = wrap_pi(p[6] - 2 * kPi * lap);
    const double xd = ref0[0], yd = ref0[1], psid = ref0[2];
    const double ey = -(p[0] - xd) * sin(psid) + (p[1] - yd) * cos(psid);
    const double epsi = wrap_pi(psi - psid);
    const double s = SS + ((vx * cos(epsi) - vy * sin(epsi)) / (1 - ey * cv0)) * c.dt;
    ls[0] = vx; ls[1] = vy; ls[2] = p[7]; ls[3] = epsi; ls[4] = s; ls[5] = ey;
}

// planner's first tick (PMAIN:137-141, :152-162, seed of PMAIN:465-505); c is the planner's configuration.  x0 [5],
// xlast [N][6], delta [N] of one vehicle.  track_view.hpp restates it on a view.  One source was tried (this body forced inline into two
// `inline` forwards of these signatures, on a table pointer and as a template over the track source): race.o and track_race.o call
// plan_first_one as a function of its own, and in both attempts that function kept its instruction count (1896 in race.o, 1901 in
// track_race.o) but had one instruction, the seed loop's v_lshl_add_u64 of the xlast row pointer, scheduled one place later; no kernel
// moved, handoff.o (where it is inlined) stayed identical
__device__ inline void plan_first_one(const DevCfg &c, const double *p, double hw, double slack, int q9_swap, double accel_rate,
                                      double *x, double *xlast, double *delta) {
    const int N = c.N;
    double s, ey, epsi; int inside;
    local_position(c, hw, slack, p[0], p[1], p[6], s, ey, epsi, inside);
    x[0] = p[2]; x[1] = p[3]; x[2] = p[7]; x[3] = q9_swap ? epsi : ey; x[4] = q9_swap ? ey : epsi;
    double vx = x[0], S = 0.0;
    for (int i = 0; i < N; ++i) {
        double *r = xlast + (size_t)i * 6;
        r[0] = vx; r[1] = x[1]; r[2] = x[2]; r[3] = x[3]; r[4] = x[4]; r[5] = S;
        delta[i] = 0.0;
        S = S + ((vx * cos(x[4]) - x[1] * sin(x[4])) / (1 - x[3] * 0)) * c.dt;
        vx = vx + (0.1 + accel_rate * i) * c.dt;
    }
}

}  // namespace lpvmpc
