// interactions.hip -- the interactions (include/lpvmpc.h, "Interactions"): slipstream and contact response between the vehicles of a
// heat, on the plant side.  One kernel in front of the tick's command / plant kernel, which it leaves as it is (as disturbance.hip).
// One workgroup per heat, as heats.hip.  Phase 1: thread i takes member i and stages what the pairwise pass needs in LDS, a struct of
// arrays (seven f64 arrays and one i32 array: 15 KB at 256 members).  One barrier.  Phase 2: thread i runs ONE loop over the n members;
// every lane reads the same LDS address in a trip, so each read is a broadcast without bank conflicts.  The wake and overlap DECISIONS
// of a trip are plain mask arithmetic; the impulse sits behind its decision, so a wavefront none of whose lanes is in contact on that
// trip skips it (the compiler speculates the shelter's two divisions into the straight path).  The loop keeps the max and argmax of
// the shelter, the sums of du and dc in ascending member order and the hit flag.  Everything is computed from the staged (pre-tick)
// words, so the result does not depend on which pair is handled first (a Jacobi step); each thread writes only its own vehicle's
// plant row, live mu word, outputs and carry: no atomics, no traffic between workgroups.
//
// Its own translation unit, compiled with -ffp-contract=off as heats.o: every product and sum of the model is rounded on its own, and
// sep comes out the same word in both vehicles of a pair and the same word as the heats'.  Two block sizes, 64 and 256 threads, chosen
// by the heats' block.  The race and the batch call launch the same kernel on their own arrays (InterDev).
#include "interactions.hpp"

namespace lpvmpc {

namespace {

template <int BS> struct InterLds {
    double x[BS], y[BS], c[BS], s[BS], ux[BS], uy[BS], m[BS];
    int32_t veh[BS];            // vehicle index of a participant, ~index (negative) of a member that does not take part
};

// one tick of heat blockIdx.x for member slot i (active: i < n) whose vehicle is b.  Every thread of the block calls it: it holds the
// block's barrier
template <int BS>
__device__ __forceinline__ void interaction_tick(const InterDev &h, InterLds<BS> &l, int t, int n, int i, bool active, int b) {
    const size_t B = h.B;
    double *p = h.plant + (size_t)b * 8;
    bool part = false;
    double x = 0, y = 0, cs = 1, sn = 0, ux = 0, uy = 0, m = 1, mu = 0;
    if (active) {
        const int ns = h.nstep ? h.nstep[b] : 1;
        const double vx = p[2], vy = p[3], yaw = p[6], inf = __builtin_inf();
        x = p[0]; y = p[1];
        part = ns > 0 && fabs(x) < inf && fabs(y) < inf && fabs(yaw) < inf && fabs(vx) < inf && fabs(vy) < inf;
        sincos(yaw, &sn, &cs);
        const double a0 = cs * vx, a1 = sn * vy, a2 = sn * vx, a3 = cs * vy;
        ux = a0 - a1; uy = a2 + a3;
        m = h.m[b]; mu = h.mu_base[b];
        l.x[i] = x; l.y[i] = y; l.c[i] = cs; l.s[i] = sn; l.ux[i] = ux; l.uy[i] = uy; l.m[i] = m;
        l.veh[i] = part ? b : ~b;
    }
    __syncthreads();
    if (!active) return;
    double *cf = h.carry_f + b, *of = h.out_f + b;
    int32_t *ci = h.carry_i + b, *oi = h.out_i + b;
    double total = cf[LPVMPC_INTER_CARRY_IMPULSE_TOTAL * B];
    int hit_ticks = ci[LPVMPC_INTER_CARRY_HIT_TICKS * B], first_hit = ci[LPVMPC_INTER_CARRY_FIRST_HIT_TICK * B];
    int draft_ticks = ci[LPVMPC_INTER_CARRY_DRAFT_TICKS * B];
    double best = 0.0, imp = 0.0;
    int leader = -1, hit = 0;
    if (part) {
        const double WL = h.wake_length, WH = h.wake_half_width, hl = h.hl, hw = h.hwc;
        const bool contact = h.contact != 0;
        double sdux = 0.0, sduy = 0.0, sdcx = 0.0, sdcy = 0.0;
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            const int wj = l.veh[j];
            const bool pj = (wj >= 0) & (j != i);
            const double xj = l.x[j], yj = l.y[j], cj = l.c[j], sj = l.s[j];
            // slipstream: i in j's wake
            const double dx = x - xj, dy = y - yj;
            const double lon = -(dx * cj + dy * sj);
            const double lat = -dx * sj + dy * cj, alat = fabs(lat);
            const double align = cs * cj + sn * sj;
            const bool wake = pj & (lon > 0) & (lon < WL) & (alat < WH) & (align > 0);
            if (wake) {
                const double w = (1.0 - lon / WL) * (1.0 - alat / WH);
                if (w > best) { best = w; leader = wj; }                    // ascending j: the lowest index attaining the max
            }
            // contact: footprint_sep of heats.hip restated (the lower index is the first rectangle, a), keeping which gap is the
            // largest and the signed projection behind it.  One function that returns the four gaps and projections to both files
            // was tried: interaction_tick_kernel<64> 1190 -> 1214 and <256> 1191 -> 1215 instructions, and in heats.o the six kernels
            // (heat_tick_kernel, heat_tick_trk_kernel, heat_step_kernel, each <64> and <256>) gained one or two each
            const bool lo = j < i;
            const double xa = lo ? xj : x, ya = lo ? yj : y, ca = lo ? cj : cs, sa = lo ? sj : sn;
            const double xb = lo ? x : xj, yb = lo ? y : yj, cb = lo ? cs : cj, sb = lo ? sn : sj;
            const double ex = xb - xa, ey = yb - ya;
            const double C = fabs(ca * cb + sa * sb), S = fabs(sa * cb - ca * sb);
            const double rl = hl + (hl * C + hw * S), rw = hw + (hl * S + hw * C);
            const double p0 = ex * ca + ey * sa, p1 = ey * ca - ex * sa, p2 = ex * cb + ey * sb, p3 = ey * cb - ex * sb;
            const double g0 = fabs(p0) - rl, g1 = fabs(p1) - rw, g2 = fabs(p2) - rl, g3 = fabs(p3) - rw;
            double sep = g0, pk = p0, ax = ca, ay = sa;                     // axes u_a, v_a, u_b, v_b: the first that attains the max
            if (g1 > sep) { sep = g1; pk = p1; ax = -sa; ay = ca; }
            if (g2 > sep) { sep = g2; pk = p2; ax = cb; ay = sb; }
            if (g3 > sep) { sep = g3; pk = p3; ax = -sb; ay = cb; }
            const bool over = pj & contact & (sep < 0);
            if (over) {
                const double sg = pk < 0 ? -1.0 : 1.0, nx = ax * sg, ny = ay * sg;   // from a to b
                const double uxj = l.ux[j], uyj = l.uy[j], mj = l.m[j];
                const double uax = lo ? uxj : ux, uay = lo ? uyj : uy, ubx = lo ? ux : uxj, uby = lo ? uy : uyj;
                const double ma = lo ? mj : m, mb = lo ? m : mj;
                const double vn = (ubx - uax) * nx + (uby - uay) * ny;
                const double J = vn < 0 ? (-(1.0 + h.restitution) * vn) / (1.0 / ma + 1.0 / mb) : 0.0;
                const double q = J / m;                                     // i is b when lo: +(J / m_b) n, else -(J / m_a) n
                const double k = (h.push * -sep) * (mj / (ma + mb));
                const double qx = q * nx, qy = q * ny, kx = k * nx, ky = k * ny;
                sdux += lo ? qx : -qx; sduy += lo ? qy : -qy;
                sdcx += lo ? kx : -kx; sdcy += lo ? ky : -ky;
                imp += fabs(J);
                hit = 1;
            }
        }
        const double mu_live = mu * (1.0 - h.draft_gain * best);
        h.mu_live[b] = mu_live;
        if (hit) {                                                          // without a partner every state word stays as it is
            const double uxn = ux + sdux, uyn = uy + sduy;
            const double vxn = cs * uxn + sn * uyn;
            p[2] = vxn > 0 ? vxn : 0.0;
            p[3] = -sn * uxn + cs * uyn;
            p[0] = x + sdcx; p[1] = y + sdcy;
        }
        total += imp;
        hit_ticks += hit;
        if (hit && first_hit < 0) first_hit = t;
        draft_ticks += best > 0;
        of[LPVMPC_INTER_MU * B] = mu_live;
        cf[LPVMPC_INTER_CARRY_IMPULSE_TOTAL * B] = total;
        ci[LPVMPC_INTER_CARRY_HIT_TICKS * B] = hit_ticks; ci[LPVMPC_INTER_CARRY_FIRST_HIT_TICK * B] = first_hit;
        ci[LPVMPC_INTER_CARRY_DRAFT_TICKS * B] = draft_ticks;
    }
    // (a member that does not take part: shelter 0, leader -1, no hit, its carried words and its MU word as they were)
    of[LPVMPC_INTER_SHELTER * B] = best; of[LPVMPC_INTER_IMPULSE * B] = imp; of[LPVMPC_INTER_IMPULSE_TOTAL * B] = total;
    oi[LPVMPC_INTER_LEADER * B] = leader; oi[LPVMPC_INTER_HIT * B] = hit; oi[LPVMPC_INTER_HIT_TICKS * B] = hit_ticks;
    oi[LPVMPC_INTER_FIRST_HIT_TICK * B] = first_hit; oi[LPVMPC_INTER_DRAFT_TICKS * B] = draft_ticks;
}

}  // namespace

template <int BS> __global__ void __launch_bounds__(BS) interaction_tick_kernel(InterDev h, int t) {
    __shared__ InterLds<BS> l;
    // the heat's slice of the member list; a heat larger than the block (the host refuses it) is cut to the block
    const int g = blockIdx.x, o = h.off[g];
    int n = h.off[g + 1] - o;
    if (n > BS) n = BS;
    const bool active = (int)threadIdx.x < n;
    const int b = active ? h.members[o + threadIdx.x] : 0;
    interaction_tick<BS>(h, l, t, n, threadIdx.x, active, b);
}

hipError_t launch_interaction_tick(const InterDev &h, int block, int t, hipStream_t s) {
    if (h.n_heats <= 0) return hipSuccess;
    const dim3 grid(h.n_heats);
    if (block <= 64) hipLaunchKernelGGL(interaction_tick_kernel<64>, grid, dim3(64), 0, s, h, t);
    else hipLaunchKernelGGL(interaction_tick_kernel<256>, grid, dim3(256), 0, s, h, t);
    return hipGetLastError();
}

}  // namespace lpvmpc
