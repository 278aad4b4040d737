// walls.hip -- the walls (include/lpvmpc.h, "Walls"): barrier contact at the track's edges, on the plant side.  One kernel in front
// of the tick's command / plant kernel, which it leaves as it is (as disturbance.hip and interactions.hip).
//
// Four lanes serve one vehicle, one corner of its footprint per lane: the cost is the search over the track's rows (two or three
// atan2 and a square root or two per row, all f64), and the four searches are independent.  Lane k of a quad locates corner k on every
// row and keeps the accepted row with the smallest |ey| (the first on a tie); the centre's search, which only OUTSIDE needs, is split
// over the quad, lane k taking rows k, k + 4, ...  The deepest corner is then chosen inside the quad with DPP quad moves (wave_ops.hpp,
// dpp_mov): the max of the four depths, the four "attains it" flags, the lowest index among them.  No LDS, no atomics, no barrier;
// ties go to the lowest corner index, so reruns are bit-identical.  The lane of the contact corner holds everything the response needs
// (its own r, ey, th) and does it; lane 0 writes the outputs of a vehicle without a contact.  Each quad writes only its own vehicle's
// plant row, outputs and carry.
//
// 256-thread workgroups, 64 vehicles each, the last one partial: the lanes of a quad beyond B stay in the kernel to the end (a quad is
// all valid or all not, so the DPP moves never read a lane that left).  Without tracks bound every lane reads the same row address on
// a trip of the corner search (a scalar or broadcast load); with tracks bound the reads go through TrackView (divergent, cached).
//
// Its own translation unit, compiled with -ffp-contract=off as interactions.o: every product and sum of the model is rounded on its
// own.  row_locate restates the row arithmetic of local_position (track_geometry.hpp / track_view.hpp) -- the straight and arc
// branches with compute_angle and norm2 of that header -- with (ey, th) as results, no s / epsi, the caller's bound and no early exit.
// One row function for both (local_position as a loop over it, epsi from its th) was tried: it moved all fifteen objects that inline
// local_position, each kernel by about 1100 instructions (local_position_kernel 1612 -> 2741, race_record_kernel 2048 -> 3158), and
// wall_tick_kernel 4271 -> 4321.
#include "walls.hpp"
#include "wave_ops.hpp"

namespace lpvmpc {

namespace {

// row i of table T (rows in use: rows) for the point (x, y): true when the row sees the point and |ey| <= bound.  local_position's
// arithmetic for one row restated; th the centreline heading at the point's foot
__device__ __forceinline__ bool row_locate(const double *T, int rows, int i, double x, double y, double bound, double &ey, double &th) {
    const int ip = i > 0 ? i - 1 : rows - 1;                            // PointAndTangent[i - 1] wraps to the last row
    const double xf = T[i * 6 + 0], yf = T[i * 6 + 1], xs = T[ip * 6 + 0], ys = T[ip * 6 + 1];
    const double ang = T[ip * 6 + 2], cv = T[i * 6 + 5];
    const bool at_s = norm2(xs - x, ys - y) == 0, at_f = norm2(xf - x, yf - y) == 0;
    ey = 0.0; th = ang;
    if (cv == 0.0) {                                                    // straight segment
        if (at_s || at_f) return true;
        if (fabs(compute_angle(x, y, xs, ys, xf, yf)) <= kPi / 2 && fabs(compute_angle(x, y, xf, yf, xs, ys)) <= kPi / 2) {
            const double n1 = norm2(x - xs, y - ys);
            const double a = compute_angle(xf, yf, xs, ys, x, y);
            ey = n1 * sin(a);
            return fabs(ey) <= bound;
        }
        return false;
    }
    if (at_s) return true;
    if (at_f) { th = T[i * 6 + 2]; return true; }
    const double r = 1 / cv;
    const double d = r >= 0 ? 1.0 : -1.0;
    const double cx = xs + fabs(r) * cos(ang + d * kPi / 2), cy = ys + fabs(r) * sin(ang + d * kPi / 2);
    const double arc1 = T[i * 6 + 4] * cv;
    const double arc2 = compute_angle(xs, ys, cx, cy, x, y);
    const double s1 = arc1 > 0 ? 1.0 : (arc1 < 0 ? -1.0 : 0.0), s2 = arc2 > 0 ? 1.0 : (arc2 < 0 ? -1.0 : 0.0);
    if (s1 == s2 && fabs(arc1) >= fabs(arc2)) {
        ey = -d * (norm2(x - cx, y - cy) - fabs(r));
        th = ang + arc2;
        return fabs(ey) <= bound;
    }
    return false;
}

template <int CTRL> __device__ __forceinline__ int dpp_movi(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }

}  // namespace

__global__ void __launch_bounds__(256) wall_tick_kernel(WallDev h, int t) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int b = gid >> 2, k = gid & 3;                                // vehicle and corner of this lane
    const bool valid = b < h.B;
    const size_t B = h.B, bb = valid ? b : 0;
    double *p = h.plant + bb * 8;
    const double x = p[0], y = p[1], vx = p[2], vy = p[3], yaw = p[6], w = p[7], inf = __builtin_inf();
    const int ns = h.nstep ? h.nstep[bb] : 1;
    const bool part = valid && ns > 0 && fabs(x) < inf && fabs(y) < inf && fabs(yaw) < inf && fabs(vx) < inf && fabs(vy) < inf && fabs(w) < inf;
    // the vehicle's track
    const double *T = h.tab;
    int rows = h.rows;
    double hw = h.hw;
    if (h.trk.tab) {
        double slack;
        const TrackView v = track_view(h.trk, (int)bb, hw, slack);
        T = v.T; rows = v.rows;
    }
    const double wall_ey = hw + h.margin, bound = wall_ey + h.reach;
    double sn = 0.0, cs = 1.0, rx = 0.0, ry = 0.0, best_ey = 0.0, best_th = 0.0, depth = 0.0;
    int located = 0, centre = 0;
    if (part) {                                                         // uniform over the quad
        sincos(yaw, &sn, &cs);
        const double a = (k & 2) ? -h.hl : h.hl, q = (k & 1) ? -h.hwc : h.hwc;
        rx = cs * a - sn * q; ry = sn * a + cs * q;
        const double px = x + rx, py = y + ry;
        double best = inf;
        for (int i = 0; i < rows; ++i) {
            double ey, th;
            if (row_locate(T, rows, i, px, py, bound, ey, th) && fabs(ey) < best) { best = fabs(ey); best_ey = ey; best_th = th; located = 1; }
        }
        for (int i = k; i < rows; i += 4) {                             // the centre, a quarter of the rows per lane
            double ey, th;
            if (row_locate(T, rows, i, x, y, bound, ey, th)) centre = 1;
        }
        if (located && fabs(best_ey) > wall_ey) depth = fabs(best_ey) - wall_ey;
    }
    // the deepest corner of the quad, the first that attains it; every lane of the wavefront is here
    double dmax = fmax(depth, dpp_mov<0xB1>(depth));                    // quad_perm [1,0,3,2]
    dmax = fmax(dmax, dpp_mov<0x4E>(dmax));                             // quad_perm [2,3,0,1]
    const int win = depth > 0.0 && depth == dmax;
    const int w0 = dpp_movi<0x00>(win), w1 = dpp_movi<0x55>(win), w2 = dpp_movi<0xAA>(win), w3 = dpp_movi<0xFF>(win);
    const int kwin = w0 ? 0 : w1 ? 1 : w2 ? 2 : w3 ? 3 : -1;
    int cen = centre | dpp_movi<0xB1>(centre);
    cen |= dpp_movi<0x4E>(cen);
    if (!valid || k != (kwin < 0 ? 0 : kwin)) return;                   // the writing lane of the quad goes on
    double *cf = h.carry_f + b, *of = h.out_f + b;
    int32_t *ci = h.carry_i + b, *oi = h.out_i + b;
    double total = cf[LPVMPC_WALL_CARRY_IMPULSE_TOTAL * B], most = cf[LPVMPC_WALL_CARRY_MAX_IMPULSE * B];
    int hit_ticks = ci[LPVMPC_WALL_CARRY_HIT_TICKS * B], first_hit = ci[LPVMPC_WALL_CARRY_FIRST_HIT_TICK * B];
    double imp = 0.0;
    int side = 0;
    if (kwin >= 0) {
        const double m = h.m[b], Iz = h.Iz[b];
        const double sth = sin(best_th), cth = cos(best_th);
        const double sd = best_ey > 0 ? 1.0 : -1.0;
        side = best_ey > 0 ? 1 : -1;
        const double nx = sd * sth, ny = -(sd * cth), tx = -ny, ty = nx;
        const double ux = cs * vx - sn * vy, uy = sn * vx + cs * vy;
        if (!h.yaw_response) { rx = 0.0; ry = 0.0; }
        // normal impulse
        const double vcx = ux + w * -ry, vcy = uy + w * rx;
        const double vn = vcx * nx + vcy * ny;
        const double rn = rx * ny - ry * nx;
        const double kn = 1.0 / m + (rn * rn) / Iz;
        const double Jn = vn < 0 ? (-(1.0 + h.restitution) * vn) / kn : 0.0;
        const double qn = Jn / m;
        const double ux1 = ux + qn * nx, uy1 = uy + qn * ny, w1 = w + (rn * Jn) / Iz;
        // friction impulse, from the velocity after the normal impulse
        const double vdx = ux1 + w1 * -ry, vdy = uy1 + w1 * rx;
        const double vt = vdx * tx + vdy * ty;
        const double rt = rx * ty - ry * tx;
        const double kt = 1.0 / m + (rt * rt) / Iz;
        const double lim = h.friction * Jn;
        double Jt = -vt / kt;
        if (Jt > lim) Jt = lim;
        if (Jt < -lim) Jt = -lim;
        const double qt = Jt / m;
        const double ux2 = ux1 + qt * tx, uy2 = uy1 + qt * ty, w2 = w1 + (rt * Jt) / Iz;
        const double vxn = cs * ux2 + sn * uy2;
        const double k2 = h.push * depth;
        p[2] = vxn > 0 ? vxn : 0.0;
        p[3] = -sn * ux2 + cs * uy2;
        if (h.yaw_response) p[7] = w2;
        p[0] = x + k2 * nx; p[1] = y + k2 * ny;
        imp = fabs(Jn);
        total += imp;
        if (imp > most) most = imp;
        hit_ticks += 1;
        if (first_hit < 0) first_hit = t;
        cf[LPVMPC_WALL_CARRY_IMPULSE_TOTAL * B] = total; cf[LPVMPC_WALL_CARRY_MAX_IMPULSE * B] = most;
        ci[LPVMPC_WALL_CARRY_HIT_TICKS * B] = hit_ticks; ci[LPVMPC_WALL_CARRY_FIRST_HIT_TICK * B] = first_hit;
    }
    // (a vehicle that does not take part: zeros and -1, its carried words as they were)
    of[LPVMPC_WALL_DEPTH * B] = kwin >= 0 ? depth : 0.0; of[LPVMPC_WALL_IMPULSE * B] = imp;
    of[LPVMPC_WALL_IMPULSE_TOTAL * B] = total; of[LPVMPC_WALL_MAX_IMPULSE * B] = most;
    oi[LPVMPC_WALL_HIT * B] = kwin >= 0; oi[LPVMPC_WALL_SIDE * B] = side; oi[LPVMPC_WALL_CORNER * B] = kwin;
    oi[LPVMPC_WALL_HIT_TICKS * B] = hit_ticks; oi[LPVMPC_WALL_FIRST_HIT_TICK * B] = first_hit;
    oi[LPVMPC_WALL_OUTSIDE * B] = part && !cen;
}

hipError_t launch_wall_tick(const WallDev &h, int t, hipStream_t s) {
    if (h.B <= 0) return hipSuccess;
    const dim3 grid((h.B + 63) / 64);
    hipLaunchKernelGGL(wall_tick_kernel, grid, dim3(256), 0, s, h, t);
    return hipGetLastError();
}

}  // namespace lpvmpc
