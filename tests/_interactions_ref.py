"""Numpy restatement of the interactions (include/lpvmpc.h, "Interactions"), written from the definitions, not from the kernel.

Two parts, as tests/_heats_ref.py.  The DECISIONS -- who takes part, who is in whose wake, which footprints overlap, which axis is the
contact axis, the sign of the normal, which leader attains the max -- are evaluated in numpy.longdouble, and ``margin`` is the smallest
distance of any of them from its threshold: a scene whose margin is at least 1e-6 is decided alike by any float64 evaluation.  The
VALUES -- shelter, the live mu, impulses, the new plant words -- are float64 with the header's operation order, every product and sum
rounded on its own, so a device whose cos / sin are the host's (every heading exactly 0) must give the same words."""
import numpy as np

from tests import _heats_ref as HR

LD = np.longdouble

F64_NAMES = ("shelter", "mu", "impulse", "impulse_total")
I32_NAMES = ("leader", "hit", "hit_ticks", "first_hit_tick", "draft_ticks")
DEFAULTS = dict(draft_gain=0.3, wake_length=3.0, wake_half_width=0.3, contact=1, restitution=0.2, push=0.5)


def config(**words):
    c = dict(DEFAULTS)
    c.update(words)
    return c


def new_carry(B):
    return dict(impulse_total=np.zeros(B), hit_ticks=np.zeros(B, int), first_hit_tick=np.full(B, -1, int), draft_ticks=np.zeros(B, int))


def participants(plant, heat, nstep=None):
    plant = np.asarray(plant, float)
    ns = np.ones(plant.shape[0], int) if nstep is None else np.asarray(nstep, int)
    return (np.asarray(heat) >= 0) & (ns > 0) & np.isfinite(plant[:, [0, 1, 6, 2, 3]]).all(axis=1)


def _decide(P, cfg, hl, hw):
    """Decisions among the n participants of one heat, P [n, 8] in member order, in long double: wake [n, n] (i in j's wake), over
    [n, n] (symmetric), and the smallest margin of any decision (inf without one)."""
    n = P.shape[0]
    x, y, th = (P[:, k].astype(LD) for k in (0, 1, 6))
    c, s = np.cos(th), np.sin(th)
    WL, WH = LD(cfg["wake_length"]), LD(cfg["wake_half_width"])
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    lon = -(dx * c[None, :] + dy * s[None, :])
    lat = np.abs(-dx * s[None, :] + dy * c[None, :])
    align = c[:, None] * c[None, :] + s[:, None] * s[None, :]
    off = ~np.eye(n, dtype=bool)
    wake = off & (lon > 0) & (lon < WL) & (lat < WH) & (align > 0)
    # a wake decision's margin: the distance of the nearest violated-or-held bound, where the other bounds do not already decide it
    d_lon = np.minimum(np.abs(lon), np.abs(lon - WL)); d_lat = np.abs(lat - WH); d_al = np.abs(align)
    held = [(lon > 0) & (lon < WL), lat < WH, align > 0]
    dist = [d_lon, d_lat, d_al]
    m_in = np.minimum(np.minimum(d_lon, d_lat), d_al)                      # inside: every bound must hold by the margin
    m_out = np.zeros((n, n), LD)                                           # outside: the violated bound that is violated by the most
    for h_, d_ in zip(held, dist):
        m_out = np.maximum(m_out, np.where(h_, 0, d_))
    m_wake = np.where(wake, m_in, m_out)
    margin = float(m_wake[off].min()) if n > 1 else np.inf
    over = np.zeros((n, n), bool)
    if n > 1:
        sep, _ = HR.sep_matrix(P[:, [0, 1, 6]], hl, hw)
        over = off & (sep < 0)
        margin = min(margin, float(np.abs(sep[off]).min()))
    return wake, over, margin


def _axis_margin(pa, pb, hl, hw):
    """Of an overlapping pair (pa the lower index), in long double: how far the contact axis' gap lies above the gaps of the axes that
    are not the same axis, and how far its projection lies from 0."""
    xa, ya, ta = (LD(v) for v in pa)
    xb, yb, tb = (LD(v) for v in pb)
    dx, dy = xb - xa, yb - ya
    ca, sa, cb, sb = np.cos(ta), np.sin(ta), np.cos(tb), np.sin(tb)
    C, S = abs(ca * cb + sa * sb), abs(sa * cb - ca * sb)
    rl, rw = LD(hl) + (LD(hl) * C + LD(hw) * S), LD(hw) + (LD(hl) * S + LD(hw) * C)
    p = [dx * ca + dy * sa, dy * ca - dx * sa, dx * cb + dy * sb, dy * cb - dx * sb]
    g = [abs(p[0]) - rl, abs(p[1]) - rw, abs(p[2]) - rl, abs(p[3]) - rw]
    k = int(np.argmax([float(v) for v in g]))
    same = float(pa[2]) == float(pb[2])                                    # equal headings: axes 0 / 2 and 1 / 3 are one axis each
    others = [q for q in range(4) if q != k and not (same and q % 2 == k % 2)]
    return min([float(g[k] - g[q]) for q in others] + [float(abs(p[k]))])


def tick(plant, rows, heat, cfg, t=0, nstep=None, carry=None, half_length=0.4, half_width=0.2):
    """One tick.  plant [B, 8], rows [B, 7] plant rows, heat [B] (-1: none), cfg a dict of words.  Returns a dict: plant (after),
    mu_live [B] (the base word where the vehicle does not take part), the named outputs, carry, written [B] (plant row rewritten),
    part [B] and margin (the smallest decision margin of the scene)."""
    plant = np.array(plant, float)
    rows = np.asarray(rows, float)
    heat = np.asarray(heat, int)
    B = plant.shape[0]
    hl, hw = float(half_length), float(half_width)
    k = new_carry(B) if carry is None else {a: np.array(b) for a, b in carry.items()}
    part = participants(plant, heat, nstep)
    out = dict(shelter=np.full(B, np.nan), mu=np.full(B, np.nan), impulse=np.full(B, np.nan), impulse_total=np.full(B, np.nan),
               leader=np.full(B, -1), hit=np.zeros(B, int), hit_ticks=np.zeros(B, int), first_hit_tick=np.full(B, -1), draft_ticks=np.zeros(B, int))
    member = heat >= 0
    out["shelter"][member] = 0.0; out["impulse"][member] = 0.0; out["mu"][member] = rows[member, 6]
    mu_live = rows[:, 6].copy()
    new = plant.copy()
    written = np.zeros(B, bool)
    margin = np.inf
    gain, WL, WH = float(cfg["draft_gain"]), float(cfg["wake_length"]), float(cfg["wake_half_width"])
    e, push = float(cfg["restitution"]), float(cfg["push"])
    for g in sorted(set(heat[member].tolist())):
        veh = np.nonzero((heat == g) & part)[0]                            # ascending: the member order
        n = veh.shape[0]
        if n == 0:
            continue
        P = plant[veh]
        x, y, vx, vy, yaw = P[:, 0], P[:, 1], P[:, 2], P[:, 3], P[:, 6]
        c, s = np.cos(yaw), np.sin(yaw)
        ux, uy = c * vx - s * vy, s * vx + c * vy
        m, mu = rows[veh, 2], rows[veh, 6]
        wake, over, mg = _decide(P, cfg, hl, hw)
        margin = min(margin, mg)
        # slipstream, float64 in the header's order; [i, j]: i in j's wake
        dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
        lon = -(dx * c[None, :] + dy * s[None, :])
        alat = np.abs(-dx * s[None, :] + dy * c[None, :])
        w = np.where(wake, (1.0 - lon / WL) * (1.0 - alat / WH), 0.0)
        for i in range(n):
            b = veh[i]
            best = float(w[i].max()) if n > 1 else 0.0
            lead = -1
            if best > 0:
                lead = int(veh[int(np.argmax(w[i]))])                      # argmax: the first, the lowest index
                rest = np.sort(w[i])[::-1]
                if n > 2 and rest[1] != rest[0]:
                    margin = min(margin, float(rest[0] - rest[1]))
            sdu, sdc, imp, hit = [0.0, 0.0], [0.0, 0.0], 0.0, 0
            if cfg["contact"]:
                for j in np.nonzero(over[i])[0]:                           # ascending partners
                    a, q = (j, i) if j < i else (i, j)                     # a: the lower index, the first rectangle
                    margin = min(margin, _axis_margin(P[a, [0, 1, 6]], P[q, [0, 1, 6]], hl, hw))
                    ex, ey = x[q] - x[a], y[q] - y[a]
                    ca, sa, cb, sb = c[a], s[a], c[q], s[q]
                    C, S = abs(ca * cb + sa * sb), abs(sa * cb - ca * sb)
                    rl, rw = hl + (hl * C + hw * S), hw + (hl * S + hw * C)
                    p = [ex * ca + ey * sa, ey * ca - ex * sa, ex * cb + ey * sb, ey * cb - ex * sb]
                    gp = [abs(p[0]) - rl, abs(p[1]) - rw, abs(p[2]) - rl, abs(p[3]) - rw]
                    axes = [(ca, sa), (-sa, ca), (cb, sb), (-sb, cb)]
                    kk = 0
                    for r in (1, 2, 3):
                        if gp[r] > gp[kk]:
                            kk = r
                    sg = -1.0 if p[kk] < 0 else 1.0
                    nx, ny = axes[kk][0] * sg, axes[kk][1] * sg
                    vn = (ux[q] - ux[a]) * nx + (uy[q] - uy[a]) * ny
                    J = -(1.0 + e) * vn / (1.0 / m[a] + 1.0 / m[q]) if vn < 0 else 0.0
                    depth = -gp[kk]
                    if i == a:
                        du = (-(J / m[a]) * nx, -(J / m[a]) * ny)
                        kq = push * depth * (m[q] / (m[a] + m[q]))
                        dc = (-kq * nx, -kq * ny)
                    else:
                        du = ((J / m[q]) * nx, (J / m[q]) * ny)
                        kq = push * depth * (m[a] / (m[a] + m[q]))
                        dc = (kq * nx, kq * ny)
                    sdu = [sdu[0] + du[0], sdu[1] + du[1]]; sdc = [sdc[0] + dc[0], sdc[1] + dc[1]]
                    imp = imp + abs(J); hit = 1
            mu_live[b] = mu[i] * (1.0 - gain * best)
            if hit:
                un = (ux[i] + sdu[0], uy[i] + sdu[1])
                new[b, 2] = max(c[i] * un[0] + s[i] * un[1], 0.0)
                new[b, 3] = -s[i] * un[0] + c[i] * un[1]
                new[b, 0] = x[i] + sdc[0]; new[b, 1] = y[i] + sdc[1]
                written[b] = True
            out["shelter"][b] = best; out["mu"][b] = mu_live[b]; out["impulse"][b] = imp; out["leader"][b] = lead; out["hit"][b] = hit
            k["impulse_total"][b] += imp; k["hit_ticks"][b] += hit; k["draft_ticks"][b] += int(best > 0)
            if hit and k["first_hit_tick"][b] < 0:
                k["first_hit_tick"][b] = t
    for name in ("impulse_total", "hit_ticks", "first_hit_tick", "draft_ticks"):
        out[name][member] = k[name][member]
    out.update(plant=new, mu_live=mu_live, carry=k, written=written, part=part, margin=float(margin))
    return out


def world_momentum(plant, rows, sel):
    """sum m u over the vehicles sel, and sum m |u| (the tolerance's scale)."""
    P = np.asarray(plant, float)[sel]
    m = np.asarray(rows, float)[sel, 2]
    c, s = np.cos(P[:, 6]), np.sin(P[:, 6])
    ux, uy = c * P[:, 2] - s * P[:, 3], s * P[:, 2] + c * P[:, 3]
    return np.array([np.sum(m * ux), np.sum(m * uy)]), float(np.sum(m * (np.abs(ux) + np.abs(uy))))


def interacting_race_ref():
    """The class of the host replay of a race with interactions attached (imported lazily: the replay needs the oracle's solver)."""
    from tests import _tyre_ref as T

    class InteractingRaceRef(T.TyreRaceRef):
        """TyreRaceRef with heats ``heat`` [B] and the interactions ``inter_cfg`` attached from tick attach_tick on.  tick() copies all
        plants at its top and computes the interaction from them; _advance applies vehicle b's share and its live mu in front of its
        simulator steps.  It raises when a vehicle it counted as a participant does not advance on that tick (a finishing or losing
        tick: the device decides participation from nstep, which the replay cannot know at the top of the tick)."""

        def __init__(self, track, plant0, heat, inter_cfg, attach_tick=0, half_length=0.4, half_width_car=0.2, **kw):
            T.TyreRaceRef.__init__(self, track, plant0, **kw)
            self.heat = np.asarray(heat, int)
            self.inter_cfg, self.attach_tick = inter_cfg, attach_tick
            self.extents = (half_length, half_width_car)
            self.inter_carry = new_carry(self.B)
            self.inter = None
            self.margin = np.inf

        def tick(self):
            self.inter = None
            if self.t >= self.attach_tick:
                steps = ((self.phase < 2) & np.isfinite(self.plant).all(axis=1)).astype(int)
                self.inter = tick(self.plant.copy(), np.array(self.rows), self.heat, self.inter_cfg, t=self.t, nstep=steps,
                                  carry=self.inter_carry, half_length=self.extents[0], half_width=self.extents[1])
                self.inter_carry = self.inter["carry"]
                self.margin = min(self.margin, self.inter["margin"])
                self._advanced = np.zeros(self.B, bool)
            T.TyreRaceRef.tick(self)
            if self.inter is not None and np.any(self.inter["part"] & ~self._advanced):
                raise RuntimeError("tick %d: vehicles %s were counted as participants and did not advance" %
                                   (self.t - 1, np.nonzero(self.inter["part"] & ~self._advanced)[0].tolist()))

        def _advance(self, b, st, n):
            if self.inter is None or not self.inter["part"][b]:
                return T.TyreRaceRef._advance(self, b, st, n)
            self._advanced[b] = True
            if self.inter["written"][b]:
                st = st.copy()
                st[[0, 1, 2, 3]] = self.inter["plant"][b, [0, 1, 2, 3]]
            base = self.rows[b].copy()
            row = base.copy(); row[6] = self.inter["mu_live"][b]
            self.rows[b] = row
            try:
                return T.TyreRaceRef._advance(self, b, st, n)
            finally:
                self.rows[b] = base

    return InteractingRaceRef
