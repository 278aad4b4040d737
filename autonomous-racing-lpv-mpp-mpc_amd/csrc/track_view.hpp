// track_view.hpp -- per-vehicle tracks (lpvmpc_set_tracks; include/lpvmpc.h, "Per-vehicle tracks"): the device view of the handle's
// track palette and the forms of the track functions that read one of its tables instead of DevCfg::track.
//   track_curvature   lpvmpc_device.hpp
//   local_position    track_geometry.hpp
//   global_position   track_geometry.hpp
// Each restates its DevCfg form with (table pointer, row count) in the place of the configuration: the same expressions in the same
// order, compiled with -ffp-contract=off like the objects of the DevCfg forms, so a palette entry equal to a handle's own table gives
// that handle's words (tests/test_gpu_tracks.py holds the pairs together, word for word).  They are restated and not shared for the
// reason veh_lpv_eval.hip gives: a second form in a translation unit moves the code of the first.
//
// The lanes of a wavefront are on different tracks, so the table reads are divergent global loads, served by the cache: the palette
// is at most kMaxTracks * 768 B = 48 KB and read-only.  Every loop is bounded by the entry's row count (<= kMaxSeg, checked when the
// binding is set) and indexed by the loop variable alone, so a lost vehicle (NaN position) reads no word outside its table: the
// comparisons fail and the function returns its sentinel.
#pragma once
#include "lpvmpc_device.hpp"
#include "track_geometry.hpp"

namespace lpvmpc {

constexpr int kMaxTracks = 64;               // = LPVMPC_MAX_TRACKS
constexpr int kTrackStride = kMaxSeg * 6;    // doubles between the tables of consecutive palette entries

// the binding on the device, passed to the kernels by value.  Vehicle b is on track of[b]; indexed by vehicle, not by launch slot
struct TrackDev {
    const double *tab;       // [T][kTrackStride] PointAndTangent rows of each entry, unused rows zero
    const int32_t *rows;     // [T] rows in use, 2 .. kMaxSeg
    const double *hw, *slack;   // [T] half width and slack of each entry
    const int32_t *of;       // [B] palette entry of each vehicle, 0 .. T-1
    int T, B;
};

// one vehicle's track: table and row count
struct TrackView {
    const double *T;
    int rows;
};
__device__ inline TrackView track_view(const TrackDev &d, int b, double &hw, double &slack) {
    const int t = d.of[b];
    hw = d.hw[t]; slack = d.slack[t];
    return TrackView{d.tab + (size_t)t * kTrackStride, d.rows[t]};
}
__device__ inline TrackView track_view(const TrackDev &d, int b) {
    const int t = d.of[b];
    return TrackView{d.tab + (size_t)t * kTrackStride, d.rows[t]};
}

// track_curvature (lpvmpc_device.hpp) on a view
__device__ inline double track_curvature(const TrackView &c, double s) {
    const int rows = c.rows;
    const double L = c.T[(rows - 1) * 6 + 3] + c.T[(rows - 1) * 6 + 4];
    s = wrap_track_s(s, L);
    for (int i = 0; i < rows; ++i) {
        const double st = c.T[i * 6 + 3], ln = c.T[i * 6 + 4];
        if (s >= st && s < st + ln) return c.T[i * 6 + 5];
    }
    return __builtin_nan("");
}

// local_position (track_geometry.hpp) on a view
__device__ __forceinline__ void local_position(const TrackView &c, double hw, double slack, double x, double y, double psi,
                                               double &s, double &ey, double &epsi, int &inside) {
    const double *T = c.T;
    const int rows = c.rows;
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

// global_position (track_geometry.hpp) on a view
__device__ inline void global_position(const TrackView &c, double s, double ey, double &x, double &y, double &th) {
    const double *T = c.T;
    const int rows = c.rows;
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

// cl_local (track_geometry.hpp) on a view: the lap-0 measurement from the plant's ground truth
__device__ __forceinline__ void cl_local(const TrackView &c, double hw, double slack, int q9_swap, const double *p, double *ls) {
    double s, ey, epsi; int inside;
    local_position(c, hw, slack, p[0], p[1], p[6], s, ey, epsi, inside);
    ls[0] = p[2] < 0.01 ? 0.01 : p[2]; ls[1] = p[3]; ls[2] = p[7];
    ls[3] = q9_swap ? ey : epsi; ls[4] = s; ls[5] = q9_swap ? epsi : ey;
}

// obs_local_state (observer_device.hpp) on a view: the controller's measurement from the estimate
__device__ inline void obs_local_state(const TrackView &c, double hw, double slack, int q9_swap, const double *e, double *ls) {
    double s, ey, epsi; int inside;
    local_position(c, hw, slack, e[3], e[4], e[5], s, ey, epsi, inside);
    ls[0] = e[0] < 0.01 ? 0.01 : e[0]; ls[1] = e[1]; ls[2] = e[2];
    ls[3] = q9_swap ? ey : epsi; ls[4] = s; ls[5] = q9_swap ? epsi : ey;
}

// plan_first_one (track_geometry.hpp) on a view; c is the planner's configuration (N, dt)
__device__ inline void plan_first_one(const DevCfg &c, const TrackView &tv, const double *p, double hw, double slack, int q9_swap,
                                      double accel_rate, double *x, double *xlast, double *delta) {
    const int N = c.N;
    double s, ey, epsi; int inside;
    local_position(tv, hw, slack, p[0], p[1], p[6], s, ey, epsi, inside);
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
