// interaction_tick.hpp -- one tick of a heat's pairwise pass, the body of interaction_tick_kernel (interactions.hip; include/lpvmpc.h,
// "Interactions") and of contact_tick_kernel (contact.hip; "Contact model"), written once ("One source, one form
// per object").  CORNER = false is the interactions' through-the-centres contact, CORNER = true the corner form: the same staging,
// barrier, loop, slipstream and overlap decision, two more staged words (w = psiDot, Iz), and behind the decision the contact point
// and the two impulses in place of the one frictionless impulse.  Everything the corner form adds stands behind `if constexpr`, so
// each object instantiates one form and interactions.o's instruction stream is the one it had when the body stood in interactions.hip
// (profiles/refactor_isa_equal.txt).
//
// Phase 1: thread i takes member i and stages what the pairwise pass needs in LDS, a struct of arrays.  One barrier.  Phase 2:
// thread i runs ONE loop over the n members; every lane reads the same LDS address in a trip, so each read is a broadcast without bank
// conflicts.  The wake and overlap DECISIONS of a trip are plain mask arithmetic; the response sits behind its decision, so a wavefront
// none of whose lanes is in contact on that trip skips it.  Everything is computed from the staged (pre-tick) words (a Jacobi step);
// each thread writes only its own vehicle's plant row, live mu word, outputs and carry: no atomics, no traffic between workgroups.
#pragma once
#include "contact.hpp"
#include "interactions.hpp"

namespace lpvmpc {

namespace {

template <int BS> struct InterLds {
    double x[BS], y[BS], c[BS], s[BS], ux[BS], uy[BS], m[BS];
    int32_t veh[BS];            // vehicle index of a participant, ~index (negative) of a member that does not take part
};
template <int BS> struct ContactLds : InterLds<BS> {
    double w[BS], iz[BS];       // psiDot and Iz of the member
};

__device__ __forceinline__ const InterDev &inter_of(const InterDev &d) { return d; }
__device__ __forceinline__ const InterDev &inter_of(const ContactDev &d) { return d.i; }

// the corner form's response of the pair (a, b) with normal n (from a to b), contact axis k and sep < 0, for the vehicle `self` of the
// pair (self_b: it is b).  Returns its du, dw and the two impulses; include/lpvmpc.h, "Contact model", in that order
struct PairBody { double x, y, c, s, ux, uy, w, m, iz; };
struct PairResponse { double dux, duy, dw, Jn, Jt; };
__device__ __forceinline__ PairResponse corner_response(const PairBody &a, const PairBody &b, bool self_b, int k, double nx, double ny, double hl,
                                                        double hw, double restitution, double friction, bool yaw_response) {
    // reference body R (owns the axis) and incident body I
    const bool Ra = k < 2;
    const double xR = Ra ? a.x : b.x, yR = Ra ? a.y : b.y, xI = Ra ? b.x : a.x, yI = Ra ? b.y : a.y;
    const double cI = Ra ? b.c : a.c, sI = Ra ? b.s : a.s;
    const double nRx = Ra ? nx : -nx, nRy = Ra ? ny : -ny, tRx = -nRy, tRy = nRx;
    const double rn = (k & 1) ? hw : hl, rt = (k & 1) ? hl : hw;
    // incident face: the first of +u, -u, +v, -v whose normal attains the min of f . n_R
    const double d0 = cI * nRx + sI * nRy, d1 = -d0, d2 = -sI * nRx + cI * nRy, d3 = -d2;
    int f = 0;
    double dm = d0;
    if (d1 < dm) { dm = d1; f = 1; }
    if (d2 < dm) { dm = d2; f = 2; }
    if (d3 < dm) { dm = d3; f = 3; }
    const double a0 = f == 1 ? -hl : hl, b0 = f == 3 ? -hw : hw, a1 = f == 0 ? hl : -hl, b1 = f == 2 ? hw : -hw;
    const double E0x = xI + (cI * a0 - sI * b0), E0y = yI + (sI * a0 + cI * b0);
    const double E1x = xI + (cI * a1 - sI * b1), E1y = yI + (sI * a1 + cI * b1);
    const double q0x = E0x - xR, q0y = E0y - yR, q1x = E1x - xR, q1y = E1y - yR;
    const double tau0 = q0x * tRx + q0y * tRy, tau1 = q1x * tRx + q1y * tRy;
    const double del0 = rn - (q0x * nRx + q0y * nRy), del1 = rn - (q1x * nRx + q1y * nRy);
    // the contact interval on the face: |tau| <= r_t and delta >= 0
    const double dt = tau1 - tau0;
    const double s1 = (rt - tau0) / dt, s2 = (-rt - tau0) / dt;
    double slo = fmax(0.0, fmin(s1, s2)), shi = fmin(1.0, fmax(s1, s2));
    bool empty = del0 < 0 && del1 < 0;
    if (!empty && (del0 < 0 || del1 < 0)) {                             // the depths differ in sign: the face leaves R on one side
        const double sd = -del0 / (del1 - del0);
        if (del0 < 0) slo = fmax(slo, sd); else shi = fmin(shi, sd);
    }
    empty = empty || slo > shi;
    const double ss = empty ? (del0 >= del1 ? 0.0 : 1.0) : (slo + shi) / 2;
    const double Px = E0x + ss * (E1x - E0x), Py = E0y + ss * (E1y - E0y);
    double rax = Px - a.x, ray = Py - a.y, rbx = Px - b.x, rby = Py - b.y;
    if (!yaw_response) { rax = 0.0; ray = 0.0; rbx = 0.0; rby = 0.0; }
    const double im = 1.0 / a.m + 1.0 / b.m;
    // normal impulse
    const double vbx = b.ux + b.w * -rby, vby = b.uy + b.w * rbx, vax = a.ux + a.w * -ray, vay = a.uy + a.w * rax;
    const double vn = (vbx - vax) * nx + (vby - vay) * ny;
    const double ka = rax * ny - ray * nx, kb = rbx * ny - rby * nx;
    const double kn = (im + (ka * ka) / a.iz) + (kb * kb) / b.iz;
    const double Jn = vn < 0 ? (-(1.0 + restitution) * vn) / kn : 0.0;
    const double qa = Jn / a.m, qb = Jn / b.m;
    const double wna = (ka * Jn) / a.iz, wnb = (kb * Jn) / b.iz;
    const double uax = a.ux - qa * nx, uay = a.uy - qa * ny, wa = a.w - wna;
    const double ubx = b.ux + qb * nx, uby = b.uy + qb * ny, wb = b.w + wnb;
    // friction impulse, from the velocities after the normal impulse
    const double tx = -ny, ty = nx;
    const double zbx = ubx + wb * -rby, zby = uby + wb * rbx, zax = uax + wa * -ray, zay = uay + wa * rax;
    const double vt = (zbx - zax) * tx + (zby - zay) * ty;
    const double la = rax * ty - ray * tx, lb = rbx * ty - rby * tx;
    const double kt = (im + (la * la) / a.iz) + (lb * lb) / b.iz;
    const double lim = friction * Jn;
    double Jt = -vt / kt;
    if (Jt > lim) Jt = lim;
    if (Jt < -lim) Jt = -lim;
    PairResponse r;
    r.Jn = Jn; r.Jt = Jt;
    if (self_b) {
        const double pt = Jt / b.m;
        r.dux = qb * nx + pt * tx; r.duy = qb * ny + pt * ty;
        r.dw = wnb + (lb * Jt) / b.iz;
    } else {
        const double pt = Jt / a.m;
        r.dux = -(qa * nx) + -(pt * tx); r.duy = -(qa * ny) + -(pt * ty);
        r.dw = -wna + -((la * Jt) / a.iz);
    }
    return r;
}

// one tick of heat blockIdx.x for member slot i (active: i < n) whose vehicle is b.  Every thread of the block calls it: it holds the
// block's barrier.  Dev / Lds: InterDev / InterLds (CORNER = false), ContactDev / ContactLds (CORNER = true)
template <int BS, bool CORNER, class Dev, class Lds>
__device__ __forceinline__ void interaction_tick(const Dev &dev, Lds &l, int t, int n, int i, bool active, int b) {
    const InterDev &h = inter_of(dev);
    const size_t B = h.B;
    double *p = h.plant + (size_t)b * 8;
    bool part = false;
    double x = 0, y = 0, cs = 1, sn = 0, ux = 0, uy = 0, m = 1, mu = 0;
    [[maybe_unused]] double w = 0, iz = 1;
    if (active) {
        const int ns = h.nstep ? h.nstep[b] : 1;
        const double vx = p[2], vy = p[3], yaw = p[6], inf = __builtin_inf();
        x = p[0]; y = p[1];
        part = ns > 0 && fabs(x) < inf && fabs(y) < inf && fabs(yaw) < inf && fabs(vx) < inf && fabs(vy) < inf;
        if constexpr (CORNER) { w = p[7]; iz = dev.Iz[b]; part = part && fabs(w) < inf; }
        sincos(yaw, &sn, &cs);
        const double a0 = cs * vx, a1 = sn * vy, a2 = sn * vx, a3 = cs * vy;
        ux = a0 - a1; uy = a2 + a3;
        m = h.m[b]; mu = h.mu_base[b];
        l.x[i] = x; l.y[i] = y; l.c[i] = cs; l.s[i] = sn; l.ux[i] = ux; l.uy[i] = uy; l.m[i] = m;
        l.veh[i] = part ? b : ~b;
        if constexpr (CORNER) { l.w[i] = w; l.iz[i] = iz; }
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
    [[maybe_unused]] double sdw = 0.0, fimp = 0.0, kick = 0.0;
    [[maybe_unused]] int partners = 0;
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
                if constexpr (!CORNER) {
                    const double uax = lo ? uxj : ux, uay = lo ? uyj : uy, ubx = lo ? ux : uxj, uby = lo ? uy : uyj;
                    const double ma = lo ? mj : m, mb = lo ? m : mj;
                    const double vn = (ubx - uax) * nx + (uby - uay) * ny;
                    const double J = vn < 0 ? (-(1.0 + h.restitution) * vn) / (1.0 / ma + 1.0 / mb) : 0.0;
                    const double q = J / m;                                 // i is b when lo: +(J / m_b) n, else -(J / m_a) n
                    const double k = (h.push * -sep) * (mj / (ma + mb));
                    const double qx = q * nx, qy = q * ny, kx = k * nx, ky = k * ny;
                    sdux += lo ? qx : -qx; sduy += lo ? qy : -qy;
                    sdcx += lo ? kx : -kx; sdcy += lo ? ky : -ky;
                    imp += fabs(J);
                } else {
                    int k = 0;                                              // the contact axis: which gap sep is
                    if (g1 > g0) k = 1;
                    if (g2 > (k ? g1 : g0)) k = 2;
                    if (g3 > (k == 2 ? g2 : k ? g1 : g0)) k = 3;
                    const PairBody me = {x, y, cs, sn, ux, uy, w, m, iz}, other = {xj, yj, cj, sj, uxj, uyj, l.w[j], mj, l.iz[j]};
                    const PairResponse r = corner_response(lo ? other : me, lo ? me : other, lo, k, nx, ny, hl, hw, h.restitution,
                                                           dev.friction, dev.yaw_response != 0);
                    const double ma = lo ? mj : m, mb = lo ? m : mj;
                    const double kp = (h.push * -sep) * (mj / (ma + mb));
                    const double kx = kp * nx, ky = kp * ny;
                    sdux += r.dux; sduy += r.duy; sdw += r.dw;
                    sdcx += lo ? kx : -kx; sdcy += lo ? ky : -ky;
                    imp += fabs(r.Jn); fimp += fabs(r.Jt); kick += fabs(r.dw);
                    partners += 1;
                }
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
            if constexpr (CORNER) {
                if (dev.yaw_response) p[7] = w + sdw;
            }
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
    if constexpr (CORNER) {                                                 // the contact model's own planes and carry
        double *kf = dev.carry_f + b, *qf = dev.out_f + b;
        int32_t *ki = dev.carry_i + b, *qi = dev.out_i + b;
        const double kick_total = kf[LPVMPC_CONTACT_CARRY_YAW_KICK_TOTAL * B] + kick;
        int most = ki[LPVMPC_CONTACT_CARRY_MAX_PARTNERS * B];
        if (partners > most) most = partners;
        if (part) { kf[LPVMPC_CONTACT_CARRY_YAW_KICK_TOTAL * B] = kick_total; ki[LPVMPC_CONTACT_CARRY_MAX_PARTNERS * B] = most; }
        qf[LPVMPC_CONTACT_FRICTION_IMPULSE * B] = fimp; qf[LPVMPC_CONTACT_YAW_KICK * B] = sdw; qf[LPVMPC_CONTACT_YAW_KICK_TOTAL * B] = kick_total;
        qi[LPVMPC_CONTACT_PARTNERS * B] = partners; qi[LPVMPC_CONTACT_MAX_PARTNERS * B] = most;
    }
}

}  // namespace

}  // namespace lpvmpc
