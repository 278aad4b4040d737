// disturbance.hip -- plant disturbances of a lap-0 fleet, a race or the stand-alone step (include/lpvmpc.h, "Plant disturbances"):
// one kernel in front of the tick's command / plant kernel, which it leaves as it is.  Per vehicle whose plant advances n > 0
// simulator steps this tick, in this order:
//   grip    the ground-truth pose on the vehicle's own track -> s; gamma = product of the patches that contain s; the live plant and
//           tyre tables' words Cf, Cr, c_f = gamma * base (the plant kernels read their tables at every simulator step)
//   gusts   a first-order Gauss-Markov process per channel (ax, ay, yaw acceleration) on the counter-based noise of
//           observer_device.hpp, keyed (seed ^ LPVMPC_DIST_STREAM, vid, j, channel), applied as an impulse d * n * dt_sim
//   kick    once, on the tick whose steps [k0, k0 + n) hold kick_step
// A frozen vehicle (n == 0) is not touched, so a vehicle's draws depend on (seed, vid, its own tick count) alone.
//   disturbance_kernel<false>   the handle's own track (DevCfg), local_position of track_geometry.hpp
//   disturbance_kernel<true>    the vehicle's palette entry (TrackDev), local_position of track_view.hpp
// One lane per vehicle, 64-lane blocks; rows, base and live tables are word-major [word][B], so a wavefront's loads of one word
// coalesce.  No LDS, no register array indexed at run time (gated: no scratch).  log / cos / sqrt run on the lanes and channels with
// sigma != 0 only.  Compiled with -ffp-contract=off like every includer of the noise generator.
#include "observer_device.hpp"
#include "track_view.hpp"

namespace lpvmpc {

template <bool kTrk> struct DistTrackArg { using type = const DevCfg *; };
template <> struct DistTrackArg<true> { using type = TrackDev; };

// channel ch of vehicle b: the process' new value from its old one (d), or d untouched where sigma == 0 (no draw)
__device__ inline double dist_gust(const DistDev &d, const double *r, size_t B, long long vid, long long j, int ch, double old, bool &on) {
    const double sigma = r[(size_t)ch * B];
    on = sigma != 0.0;
    if (!on) return old;
    double g = obs_gauss(d.seed, vid, j, ch);
    g = g > d.n_bound ? d.n_bound : (g < -d.n_bound ? -d.n_bound : g);
    if (j == 0) return sigma * g;
    return r[3 * B] * old + sigma * r[(size_t)kDistWords * B] * g;          // rho d + sigma q g, q = sqrt(1 - rho^2) from the host
}

template <bool kTrk>
__global__ void __launch_bounds__(64) disturbance_kernel(typename DistTrackArg<kTrk>::type trk, DistDev d) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= d.B) return;
    const int n = d.nstep ? d.nstep[b] : d.n_fixed;
    if (n <= 0) return;                                                     // frozen: plant, tables and tick count stay put
    const size_t B = d.B;
    const double *r = d.rows + b;
    double *p = d.plant + (size_t)b * 8, *stt = d.state + b;
    // 1. grip
    double s, ey, epsi, L;
    int inside;
    if constexpr (kTrk) {
        double hw, slack;
        const TrackView v = track_view(trk, b, hw, slack);
        local_position(v, hw, slack, p[0], p[1], p[6], s, ey, epsi, inside);
        L = v.T[(v.rows - 1) * 6 + 3] + v.T[(v.rows - 1) * 6 + 4];
    } else {
        const DevCfg &c = *trk;
        local_position(c, d.hw, d.slack, p[0], p[1], p[6], s, ey, epsi, inside);
        L = c.track[(c.track_rows - 1) * 6 + 3] + c.track[(c.track_rows - 1) * 6 + 4];
    }
    double gamma = 1.0;
    if (inside) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            double dd = s - r[(size_t)(7 + 3 * q) * B];
            if (dd < 0) dd += L;
            if (dd < r[(size_t)(8 + 3 * q) * B]) gamma *= r[(size_t)(9 + 3 * q) * B];
        }
    }
    d.live_p[4 * B + b] = gamma * d.base[b];
    d.live_p[5 * B + b] = gamma * d.base[B + b];
    d.live_t[3 * B + b] = gamma * d.base[2 * B + b];
    // 2. gusts
    const long long j = (long long)stt[3 * B], vid = d.voff + b;
    const double T = (double)n * d.dt;
    bool on;
    const double d0 = dist_gust(d, r, B, vid, j, 0, stt[0], on);
    if (on) { stt[0] = d0; p[2] = fabs(p[2] + d0 * T); }
    const double d1 = dist_gust(d, r, B, vid, j, 1, stt[B], on);
    if (on) { stt[B] = d1; p[3] = p[3] + d1 * T; }
    const double d2 = dist_gust(d, r, B, vid, j, 2, stt[2 * B], on);
    if (on) { stt[2 * B] = d2; p[7] = p[7] + d2 * T; }
    // 3. kick: once, on the tick whose steps hold kick_step (< 0: never, k0 >= 0)
    const int k0 = d.k[b];
    const double ks = r[4 * B];
    if (ks >= (double)k0 && ks < (double)k0 + (double)n) { p[3] = p[3] + r[5 * B]; p[7] = p[7] + r[6 * B]; }
    // 4.
    stt[3 * B] = (double)(j + 1);
    stt[4 * B] = gamma;
}

hipError_t launch_disturbance(const DevCfg *dcfg, const TrackDev *trk, const DistDev &d, hipStream_t s) {
    const dim3 grid((d.B + 63) / 64), block(64);
    if (trk) hipLaunchKernelGGL(disturbance_kernel<true>, grid, block, 0, s, *trk, d);
    else hipLaunchKernelGGL(disturbance_kernel<false>, grid, block, 0, s, dcfg, d);
    return hipGetLastError();
}

}  // namespace lpvmpc
