// track_view.hpp -- per-vehicle tracks (lpvmpc_set_tracks; include/lpvmpc.h, "Per-vehicle tracks"): the device view of the handle's
// track palette and the forms of the track functions that read one of its tables instead of DevCfg::track.
//   track_curvature   lpvmpc_device.hpp
//   local_position    track_geometry.hpp
//   global_position   track_geometry.hpp
//   cl_local          track_geometry.hpp
//   obs_local_state   observer_device.hpp
// Each forwards the view's (table pointer, row count) to the one source of the function, which the DevCfg form forwards to as well, so
// a palette entry equal to a handle's own table gives that handle's words (tests/test_gpu_tracks.py holds the pairs together, word
// for word).  One source is not one object: the bound kernels stay in translation units of their own, since a second form in a
// translation unit moves the code of the first ("One source, one form per object").
//
// The lanes of a wavefront are on different tracks, so the table reads are divergent global loads, served by the cache: the palette
// is at most kMaxTracks * 768 B = 48 KB and read-only.  Every loop is bounded by the entry's row count (<= kMaxSeg, checked when the
// binding is set) and indexed by the loop variable alone, so a lost vehicle (NaN position) reads no word outside its table: the
// comparisons fail and the function returns its sentinel.
#pragma once
#include "lpvmpc_device.hpp"
#include "track_geometry.hpp"
#include "observer_device.hpp"

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

// the track functions on a view: forwards to the one source of each (lpvmpc_device.hpp, track_geometry.hpp, observer_device.hpp)
__device__ __forceinline__ double track_curvature(const TrackView &c, double s) { return track_curvature(c.T, c.rows, s); }
__device__ __forceinline__ void local_position(const TrackView &c, double hw, double slack, double x, double y, double psi,
                                               double &s, double &ey, double &epsi, int &inside) {
    local_position(c.T, c.rows, hw, slack, x, y, psi, s, ey, epsi, inside);
}
__device__ __forceinline__ void global_position(const TrackView &c, double s, double ey, double &x, double &y, double &th) {
    global_position(c.T, c.rows, s, ey, x, y, th);
}
// the lap-0 measurement from the plant's ground truth
__device__ __forceinline__ void cl_local(const TrackView &c, double hw, double slack, int q9_swap, const double *p, double *ls) {
    cl_local(c.T, c.rows, hw, slack, q9_swap, p, ls);
}
// the controller's measurement from the estimate
__device__ __forceinline__ void obs_local_state(const TrackView &c, double hw, double slack, int q9_swap, const double *e, double *ls) {
    obs_local_state(c.T, c.rows, hw, slack, q9_swap, e, ls);
}
// plan_first_one (track_geometry.hpp) on a view; c is the planner's configuration (N, dt).  Restated: the comment there says what sharing
// it moved
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
