// heats.hip -- the heats (include/lpvmpc.h, "Heats"): order, gaps, passes, line crossings and footprint clearances of the vehicles
// that share a track, kept on the device.  One workgroup per heat.  Phase 1: thread i takes member i, locates it on its track
// (race form: local_position inline, as the recorder; batch form: s / inside are read), updates turns and progress and stages what
// the pairwise pass needs in LDS, a struct of arrays.  Phase 2: thread i runs ONE loop over the n members; every lane reads the same
// LDS address in a trip, so each read is a broadcast without bank conflicts, and nothing in the loop is indexed at run time into a
// register array.  The loop counts the members ordered before i (the order is total, so the counts are a permutation, which is then
// inverted through LDS to find the member in front and the leader), counts the order flips against the previous tick, and
// evaluates sep for the eligible partners.  It reads race state only and writes the heats' buffers only.
//
// Its own translation unit, compiled with -ffp-contract=off as record.o: progress = (double)turns * L + s is rounded twice, and
// the products and sums of sep come out the same in both vehicles of a pair.  Two block sizes: 64 threads (one wavefront, for a
// launch whose largest heat has at most 64 members) and 256; the host chooses when the heats are attached.
#include "heats.hpp"
#include "track_geometry.hpp"

namespace lpvmpc {

namespace {

template <int BS> struct HeatLds {
    double x[BS], y[BS], c[BS], s[BS], prog[BS], prev[BS];
    int32_t cls[BS];            // class | previous class << 8 (0xff: no previous tick) | eligible for the clearance << 16
    int32_t fin[BS];            // finish tick
    int32_t veh[BS];            // vehicle index
    int32_t inv[BS];            // member at each position
};

// a is ordered before b: (progress descending, NaN last), then member slot (= vehicle index order).  Branch-free, as the whole
// pairwise loop: plain mask arithmetic that the compiler can schedule across trips
__device__ __forceinline__ bool progress_before(double pa, int ia, double pb, int ib) {
    const bool gt = pa > pb, lt = pa < pb, na = pa != pa, nb = pb != pb;
    return gt | (!lt & ((na != nb) ? nb : (ia < ib)));
}
__device__ __forceinline__ bool order_before(int ca, int fa, double pa, int ia, int cb, int fb, double pb, int ib) {
    const bool by_finish = (ca == 0) & (fa != fb);
    return (ca < cb) | ((ca == cb) & (by_finish ? (fa < fb) : progress_before(pa, ia, pb, ib)));
}

// sep of rectangle A (first: the lower index) and B: the largest of the four separating-axis gaps
__device__ __forceinline__ double footprint_sep(double hl, double hw, double xa, double ya, double ca, double sa, double xb, double yb,
                                                double cb, double sb) {
    const double dx = xb - xa, dy = yb - ya;
    const double C = fabs(ca * cb + sa * sb), S = fabs(sa * cb - ca * sb);
    const double rl = hl + (hl * C + hw * S), rw = hw + (hl * S + hw * C);
    const double g0 = fabs(dx * ca + dy * sa) - rl;
    const double g1 = fabs(dy * ca - dx * sa) - rw;
    const double g2 = fabs(dx * cb + dy * sb) - rl;
    const double g3 = fabs(dy * cb - dx * sb) - rw;
    double m = g0;
    if (g1 > m) m = g1;
    if (g2 > m) m = g2;
    if (g3 > m) m = g3;
    return m;
}

// one tick of heat g for member slot i (active: i < n) whose vehicle b has pose (x, y, yaw), track frame (s, inside) and track
// length L.  Every thread of the block calls it: it holds the block's barriers
template <int BS>
__device__ __forceinline__ void heat_tick(const HeatDev &h, HeatLds<BS> &l, int t, int n, int i, bool active, int b, double x, double y,
                                          double yaw, double s, int inside, double L, int phase) {
    const size_t B = h.B;
    double *cf = h.carry_f + b;
    int32_t *ci = h.carry_i + b;
    int flags = 0, turns = 0, turns0 = 0, crossings = 0, fin = -1, contact_ticks = 0, first_contact = -1, passes = 0, passed = 0;
    int cls = 0, cls_prev = 0xff, line_k = -1;
    double s_last = 0.0, prog = __builtin_nan(""), prog_prev = __builtin_nan(""), min_clear = __builtin_inf();
    if (active) {
        flags = ci[LPVMPC_HEAT_CARRY_FLAGS * B];
        turns = ci[LPVMPC_HEAT_CARRY_TURNS * B];
        const int phase_prev = ci[LPVMPC_HEAT_CARRY_PHASE * B];
        turns0 = turns;
        if (flags & 1) {
            turns0 = ci[LPVMPC_HEAT_CARRY_TURNS0 * B]; crossings = ci[LPVMPC_HEAT_CARRY_CROSSINGS * B];
            fin = ci[LPVMPC_HEAT_CARRY_FINISH_TICK * B]; contact_ticks = ci[LPVMPC_HEAT_CARRY_CONTACT_TICKS * B];
            first_contact = ci[LPVMPC_HEAT_CARRY_FIRST_CONTACT * B]; passes = ci[LPVMPC_HEAT_CARRY_PASSES * B];
            passed = ci[LPVMPC_HEAT_CARRY_PASSED * B];
            s_last = cf[LPVMPC_HEAT_CARRY_S * B]; prog_prev = cf[LPVMPC_HEAT_CARRY_PROGRESS * B];
            min_clear = cf[LPVMPC_HEAT_CARRY_MIN_CLEARANCE * B];
            cls_prev = phase_prev == 2 ? 0 : phase_prev == 3 ? 3 : (flags & 2) ? 1 : 2;
        } else {
            flags = 0;
        }
        if (inside == 1 && fabs(s) < __builtin_inf()) {                 // located
            if (flags & 2) {
                const double d = s - s_last;
                if (d < -L / 2) turns += 1;
                else if (d > L / 2) turns -= 1;
            }
            s_last = s;
            flags |= 2;
        }
        if (flags & 2) { const double tl = (double)turns * L; prog = tl + s_last; }
        cls = phase == 2 ? 0 : phase == 3 ? 3 : (flags & 2) ? 1 : 2;
        if (phase == 2 && phase_prev != 2) fin = t;
        if (turns - turns0 > crossings) { line_k = crossings; crossings += 1; }
        const bool finite_pose = fabs(x) < __builtin_inf() && fabs(y) < __builtin_inf() && fabs(yaw) < __builtin_inf();
        const int elig = (cls == 1 || cls == 2) && finite_pose;
        double sn, cs;
        sincos(yaw, &sn, &cs);
        l.x[i] = x; l.y[i] = y; l.c[i] = cs; l.s[i] = sn; l.prog[i] = prog; l.prev[i] = prog_prev;
        l.cls[i] = cls | (cls_prev << 8) | (elig << 16);
        l.fin[i] = fin; l.veh[i] = b;
    }
    __syncthreads();
    int pos = 0, nearest = -1;
    double clear = __builtin_inf();
    if (active) {
        const double xi = l.x[i], yi = l.y[i], ci_ = l.c[i], si = l.s[i];
        const int elig = (l.cls[i] >> 16) & 1;
        const bool both_i = cls == 1 && cls_prev == 1;
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            const int w = l.cls[j];
            const int cj = w & 0xff, cpj = (w >> 8) & 0xff;
            const bool other = j != i;
            const bool j_first = order_before(cj, l.fin[j], l.prog[j], j, cls, fin, prog, i);
            pos += other & j_first;
            const bool pair = other & both_i & (cj == 1) & (cpj == 1);
            const bool j_was_first = progress_before(l.prev[j], j, prog_prev, i);
            passes += pair & j_was_first & !j_first;
            passed += pair & !j_was_first & j_first;
            const bool lo = j < i;                                      // the lower index is the first rectangle
            const double xj = l.x[j], yj = l.y[j], cj_ = l.c[j], sj = l.s[j];
            const double sep = footprint_sep(h.hl, h.hwc, lo ? xj : xi, lo ? yj : yi, lo ? cj_ : ci_, lo ? sj : si,
                                             lo ? xi : xj, lo ? yi : yj, lo ? ci_ : cj_, lo ? si : sj);
            const bool take = other & (elig != 0) & (((w >> 16) & 1) != 0) & (sep < clear);     // (a NaN sep of a pose-less partner never is)
            clear = take ? sep : clear;
            nearest = take ? l.veh[j] : nearest;
        }
        l.inv[pos] = i;
    }
    __syncthreads();
    if (!active) return;
    int ahead = -1;
    double gap_ahead = __builtin_nan(""), gap_leader = __builtin_nan("");
    if (pos > 0) {
        const int ja = l.inv[pos - 1] & (BS - 1), jl = l.inv[0] & (BS - 1);     // (masked: no read outside the arrays, whatever inv holds)
        ahead = l.veh[ja];
        if (cls == 1 && (l.cls[ja] & 0xff) == 1) gap_ahead = l.prog[ja] - prog;
        if (cls == 1 && (l.cls[jl] & 0xff) == 1) gap_leader = l.prog[jl] - prog;
    }
    const int contact = clear < 0;
    if (clear < min_clear) min_clear = clear;
    contact_ticks += contact;
    if (contact && first_contact < 0) first_contact = t;
    if (line_k >= 0 && line_k < h.K) { h.line_tick[(size_t)b * h.K + line_k] = t; h.line_pos[(size_t)b * h.K + line_k] = pos; }
    double *of = h.out_f + b;
    int32_t *oi = h.out_i + b;
    of[LPVMPC_HEAT_PROGRESS * B] = prog; of[LPVMPC_HEAT_GAP_AHEAD * B] = gap_ahead; of[LPVMPC_HEAT_GAP_LEADER * B] = gap_leader;
    of[LPVMPC_HEAT_CLEARANCE * B] = clear; of[LPVMPC_HEAT_MIN_CLEARANCE * B] = min_clear;
    oi[LPVMPC_HEAT_POSITION * B] = pos; oi[LPVMPC_HEAT_AHEAD * B] = ahead; oi[LPVMPC_HEAT_NEAREST * B] = nearest;
    oi[LPVMPC_HEAT_CONTACT * B] = contact; oi[LPVMPC_HEAT_CONTACT_TICKS * B] = contact_ticks;
    oi[LPVMPC_HEAT_FIRST_CONTACT_TICK * B] = first_contact; oi[LPVMPC_HEAT_PASSES * B] = passes; oi[LPVMPC_HEAT_PASSED * B] = passed;
    oi[LPVMPC_HEAT_TURNS * B] = turns; oi[LPVMPC_HEAT_CLASS * B] = cls;
    cf[LPVMPC_HEAT_CARRY_S * B] = s_last; cf[LPVMPC_HEAT_CARRY_PROGRESS * B] = prog; cf[LPVMPC_HEAT_CARRY_MIN_CLEARANCE * B] = min_clear;
    ci[LPVMPC_HEAT_CARRY_FLAGS * B] = flags | 1; ci[LPVMPC_HEAT_CARRY_TURNS * B] = turns; ci[LPVMPC_HEAT_CARRY_TURNS0 * B] = turns0;
    ci[LPVMPC_HEAT_CARRY_CROSSINGS * B] = crossings; ci[LPVMPC_HEAT_CARRY_PHASE * B] = phase; ci[LPVMPC_HEAT_CARRY_FINISH_TICK * B] = fin;
    ci[LPVMPC_HEAT_CARRY_CONTACT_TICKS * B] = contact_ticks; ci[LPVMPC_HEAT_CARRY_FIRST_CONTACT * B] = first_contact;
    ci[LPVMPC_HEAT_CARRY_PASSES * B] = passes; ci[LPVMPC_HEAT_CARRY_PASSED * B] = passed;
}

// the heat's slice of the member list; a heat larger than the block (the host refuses it) is cut to the block
template <int BS> __device__ __forceinline__ int heat_members(const HeatDev &h, int &n, bool &active) {
    const int g = blockIdx.x, o = h.off[g];
    n = h.off[g + 1] - o;
    if (n > BS) n = BS;
    active = (int)threadIdx.x < n;
    return active ? h.members[o + threadIdx.x] : 0;
}

}  // namespace

template <int BS> __global__ void __launch_bounds__(BS) heat_tick_kernel(const DevCfg *__restrict__ cp, HeatDev h, int t) {
    __shared__ HeatLds<BS> l;
    int n; bool active;
    const int b = heat_members<BS>(h, n, active);
    const DevCfg &c = *cp;
    double x = 0, y = 0, yaw = 0, s = 0, ey, epsi, L = 1;
    int inside = 0, phase = 0;
    if (active) {
        const double *p = h.plant + (size_t)b * 8;
        x = p[0]; y = p[1]; yaw = p[6]; phase = h.phase[b];
        local_position(c, h.hw, h.slack, x, y, yaw, s, ey, epsi, inside);      // the ground-truth plant's track frame
        L = c.track[(c.track_rows - 1) * 6 + 3] + c.track[(c.track_rows - 1) * 6 + 4];
    }
    heat_tick<BS>(h, l, t, n, threadIdx.x, active, b, x, y, yaw, s, inside, L, phase);
}

template <int BS> __global__ void __launch_bounds__(BS) heat_tick_trk_kernel(TrackDev trk, HeatDev h, int t) {
    __shared__ HeatLds<BS> l;
    int n; bool active;
    const int b = heat_members<BS>(h, n, active);
    double x = 0, y = 0, yaw = 0, s = 0, ey, epsi, L = 1;
    int inside = 0, phase = 0;
    if (active) {
        const double *p = h.plant + (size_t)b * 8;
        x = p[0]; y = p[1]; yaw = p[6]; phase = h.phase[b];
        double hw, slack;
        const TrackView tv = track_view(trk, b, hw, slack);
        local_position(tv, hw, slack, x, y, yaw, s, ey, epsi, inside);
        L = tv.T[(tv.rows - 1) * 6 + 3] + tv.T[(tv.rows - 1) * 6 + 4];
    }
    heat_tick<BS>(h, l, t, n, threadIdx.x, active, b, x, y, yaw, s, inside, L, phase);
}

template <int BS> __global__ void __launch_bounds__(BS) heat_step_kernel(HeatDev h, int t) {
    __shared__ HeatLds<BS> l;
    int n; bool active;
    const int b = heat_members<BS>(h, n, active);
    double x = 0, y = 0, yaw = 0, s = 0, L = 1;
    int inside = 0, phase = 0;
    if (active) {
        x = h.pose[(size_t)b * 3 + 0]; y = h.pose[(size_t)b * 3 + 1]; yaw = h.pose[(size_t)b * 3 + 2];
        s = h.s[b]; inside = h.inside[b]; L = h.L[b]; phase = h.phase[b];
    }
    heat_tick<BS>(h, l, t, n, threadIdx.x, active, b, x, y, yaw, s, inside, L, phase);
}

hipError_t launch_heat_tick(const DevCfg *ccfg, const TrackDev *trk, const HeatDev &h, int block, int t, hipStream_t s) {
    if (h.n_heats <= 0) return hipSuccess;
    const dim3 grid(h.n_heats);
    if (trk) {
        if (block <= 64) hipLaunchKernelGGL(heat_tick_trk_kernel<64>, grid, dim3(64), 0, s, *trk, h, t);
        else hipLaunchKernelGGL(heat_tick_trk_kernel<256>, grid, dim3(256), 0, s, *trk, h, t);
    } else {
        if (block <= 64) hipLaunchKernelGGL(heat_tick_kernel<64>, grid, dim3(64), 0, s, ccfg, h, t);
        else hipLaunchKernelGGL(heat_tick_kernel<256>, grid, dim3(256), 0, s, ccfg, h, t);
    }
    return hipGetLastError();
}

hipError_t launch_heat_step(const HeatDev &h, int block, int t, hipStream_t s) {
    if (h.n_heats <= 0) return hipSuccess;
    const dim3 grid(h.n_heats);
    if (block <= 64) hipLaunchKernelGGL(heat_step_kernel<64>, grid, dim3(64), 0, s, h, t);
    else hipLaunchKernelGGL(heat_step_kernel<256>, grid, dim3(256), 0, s, h, t);
    return hipGetLastError();
}

}  // namespace lpvmpc
