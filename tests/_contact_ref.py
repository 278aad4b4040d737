"""Numpy restatement of the contact model (include/lpvmpc.h, "Contact model"), written from the header, not from the kernel.

As tests/_interactions_ref.py, in two parts.  One function, ``pair``, states the response of an overlapping pair once, generic over the
number type.  It runs in numpy.longdouble to take the DECISIONS, each with its margin, and in float64, in the header's operation order
with every product and sum rounded on its own, to give the VALUES under those decisions.
  hard decisions -- a wrong one changes the result by a jump: the interactions' own (who takes part, wakes, overlaps, the contact
    axis, the sign of the normal), the incident face, and the emptiness of the contact interval (the width s_hi - s_lo of a non-empty
    one; ``empty`` counts the pairs that reached the rule for an empty interval).  ``margin`` is the smallest of them.
  clips -- max / min / clamp selections between two values that coincide at the threshold, so that a wrong one moves the result by
    no more than the distance to the threshold: whether each tau clip and each depth is active, vn < 0, each friction clamp.
    ``clip_margin`` is the smallest distance of any of them from its threshold; one that sits ON its threshold (within 1e-12: a flat,
    centred hit puts the face's end exactly on the reference body's side) selects between equal values and is not counted.
A scene whose margins are at least 1e-6 is decided alike by any float64 evaluation."""
import numpy as np

from tests import _interactions_ref as R

LD = np.longdouble
F64_NAMES = ("friction_impulse", "yaw_kick", "yaw_kick_total")
I32_NAMES = ("partners", "max_partners")
DEFAULTS = dict(friction=0.3, yaw_response=1)
TIE = 1e-12
FACE_ENDS = {0: ((1, 1), (1, -1)), 1: ((-1, 1), (-1, -1)), 2: ((1, 1), (-1, 1)), 3: ((1, -1), (-1, -1))}   # the walls' corner order


def config(**words):
    c = dict(DEFAULTS)
    c.update(words)
    return c


def new_carry(B):
    return dict(yaw_kick_total=np.zeros(B), max_partners=np.zeros(B, int))


def participants(plant, heat, nstep=None):
    return R.participants(plant, heat, nstep) & np.isfinite(np.asarray(plant, float)[:, 7])


def body(T, row, m, iz):
    """A staged participant in number type T: x, y, c, s, ux, uy, w, m, Iz from its plant row."""
    x, y, vx, vy, yaw, w = (T(row[k]) for k in (0, 1, 2, 3, 6, 7))
    c, s = np.cos(yaw), np.sin(yaw)
    return dict(x=x, y=y, c=c, s=s, ux=c * vx - s * vy, uy=s * vx + c * vy, w=w, m=T(m), iz=T(iz))


def _soft(d):
    d = abs(float(d))
    return np.inf if d <= TIE else d


def pair(T, a, b, hl, hw, e, push, friction, yaw_response, take=None):
    """The response of the pair a < b (dicts of ``body``) in number type T, None when sep >= 0.  take: the hard decisions of another
    run (k, sg, face, empty) to evaluate under; None: decide here and report the margins."""
    hl, hw, e, push, friction = T(hl), T(hw), T(e), T(push), T(friction)
    ex, ey = b["x"] - a["x"], b["y"] - a["y"]
    ca, sa, cb, sb = a["c"], a["s"], b["c"], b["s"]
    C, S = abs(ca * cb + sa * sb), abs(sa * cb - ca * sb)
    rl, rw = hl + (hl * C + hw * S), hw + (hl * S + hw * C)
    p = [ex * ca + ey * sa, ey * ca - ex * sa, ex * cb + ey * sb, ey * cb - ex * sb]
    g = [abs(p[0]) - rl, abs(p[1]) - rw, abs(p[2]) - rl, abs(p[3]) - rw]
    axes = [(ca, sa), (-sa, ca), (cb, sb), (-sb, cb)]
    if take is None:
        k = 0
        for r in (1, 2, 3):
            if g[r] > g[k]:
                k = r
        if not g[k] < 0:
            return None
        sg = T(-1.0) if p[k] < 0 else T(1.0)
    else:
        k, sg = take["k"], T(take["sg"])
    sep = g[k]
    nx, ny = axes[k][0] * sg, axes[k][1] * sg
    hard, soft = np.inf, np.inf
    # reference and incident body
    Rb, Ib = (a, b) if k < 2 else (b, a)
    nRx, nRy = (nx, ny) if k < 2 else (-nx, -ny)
    tRx, tRy = -nRy, nRx
    rn, rt = (hl, hw) if k % 2 == 0 else (hw, hl)
    cI, sI = Ib["c"], Ib["s"]
    d0 = cI * nRx + sI * nRy
    d2 = -sI * nRx + cI * nRy
    d = [d0, -d0, d2, -d2]
    if take is None:
        f = 0
        for r in (1, 2, 3):
            if d[r] < d[f]:
                f = r
        hard = min(hard, min(float(d[r] - d[f]) for r in range(4) if r != f))
    else:
        f = take["face"]
    E, tau, dl = [], [], []
    for sa_, sb_ in FACE_ENDS[f]:
        aj, bj = T(sa_) * hl, T(sb_) * hw
        Ex, Ey = Ib["x"] + (cI * aj - sI * bj), Ib["y"] + (sI * aj + cI * bj)
        qx, qy = Ex - Rb["x"], Ey - Rb["y"]
        E.append((Ex, Ey)); tau.append(qx * tRx + qy * tRy); dl.append(rn - (qx * nRx + qy * nRy))
    dt = tau[1] - tau[0]
    s1, s2 = (rt - tau[0]) / dt, (-rt - tau[0]) / dt
    slo, shi = max(T(0.0), min(s1, s2)), min(T(1.0), max(s1, s2))
    soft = min(soft, _soft(min(s1, s2)), _soft(max(s1, s2) - 1), _soft(dl[0]), _soft(dl[1]))
    empty = bool(dl[0] < 0 and dl[1] < 0)
    if not empty and (dl[0] < 0 or dl[1] < 0):
        sd = -dl[0] / (dl[1] - dl[0])
        if dl[0] < 0:
            slo = max(slo, sd)
        else:
            shi = min(shi, sd)
    if take is None:
        empty = empty or bool(slo > shi)
        hard = min(hard, abs(float(shi - slo)))
    else:
        empty = take["empty"]
    ss = (T(0.0) if dl[0] >= dl[1] else T(1.0)) if empty else (slo + shi) / 2
    Px, Py = E[0][0] + ss * (E[1][0] - E[0][0]), E[0][1] + ss * (E[1][1] - E[0][1])
    rax, ray, rbx, rby = Px - a["x"], Py - a["y"], Px - b["x"], Py - b["y"]
    if not yaw_response:
        rax = ray = rbx = rby = T(0.0)
    im = T(1.0) / a["m"] + T(1.0) / b["m"]
    # normal impulse
    vbx, vby = b["ux"] + b["w"] * -rby, b["uy"] + b["w"] * rbx
    vax, vay = a["ux"] + a["w"] * -ray, a["uy"] + a["w"] * rax
    vn = (vbx - vax) * nx + (vby - vay) * ny
    ka, kb = rax * ny - ray * nx, rbx * ny - rby * nx
    kn = (im + (ka * ka) / a["iz"]) + (kb * kb) / b["iz"]
    soft = min(soft, _soft(vn))
    Jn = (-(T(1.0) + e) * vn) / kn if vn < 0 else T(0.0)
    qa, qb = Jn / a["m"], Jn / b["m"]
    wna, wnb = (ka * Jn) / a["iz"], (kb * Jn) / b["iz"]
    uax, uay, wa = a["ux"] - qa * nx, a["uy"] - qa * ny, a["w"] - wna
    ubx, uby, wb = b["ux"] + qb * nx, b["uy"] + qb * ny, b["w"] + wnb
    # friction impulse
    tx, ty = -ny, nx
    zbx, zby = ubx + wb * -rby, uby + wb * rbx
    zax, zay = uax + wa * -ray, uay + wa * rax
    vt = (zbx - zax) * tx + (zby - zay) * ty
    la, lb = rax * ty - ray * tx, rbx * ty - rby * tx
    kt = (im + (la * la) / a["iz"]) + (lb * lb) / b["iz"]
    lim = friction * Jn
    Jt = -vt / kt
    if float(lim) > 0:
        soft = min(soft, _soft(abs(Jt) - lim))
    if Jt > lim:
        Jt = lim
    if Jt < -lim:
        Jt = -lim
    pa, pb = Jt / a["m"], Jt / b["m"]
    depth = -sep
    ka_ = push * depth * (b["m"] / (a["m"] + b["m"]))
    kb_ = push * depth * (a["m"] / (a["m"] + b["m"]))
    return dict(k=k, sg=float(sg), face=f, empty=empty, hard=hard, soft=soft, n=(nx, ny), P=(Px, Py), Jn=Jn, Jt=Jt, s=ss,
                du_a=(-(qa * nx) + -(pa * tx), -(qa * ny) + -(pa * ty)), dw_a=-wna + -((la * Jt) / a["iz"]),
                du_b=(qb * nx + pb * tx, qb * ny + pb * ty), dw_b=wnb + (lb * Jt) / b["iz"],
                dc_a=(-ka_ * nx, -ka_ * ny), dc_b=(kb_ * nx, kb_ * ny))


def respond(row_a, row_b, ma, iza, mb, izb, cfg, ccfg, hl=0.4, hw=0.2):
    """One pair, a the lower index: (float64 response under the long-double decisions, the long-double response), or (None, None)."""
    args = (hl, hw, cfg["restitution"], cfg["push"], ccfg["friction"], ccfg["yaw_response"])
    dec = pair(LD, body(LD, row_a, ma, iza), body(LD, row_b, mb, izb), *args)
    if dec is None:
        return None, None
    return pair(np.float64, body(np.float64, row_a, ma, iza), body(np.float64, row_b, mb, izb), *args, take=dec), dec


def tick(plant, rows, heat, cfg, ccfg, t=0, nstep=None, carry=None, ccarry=None, half_length=0.4, half_width=0.2):
    """One tick.  As _interactions_ref.tick, with the contact configuration ccfg and its carry; returns that function's dict plus the
    contact model's named planes, ccarry, clip_margin and empty (pairs that reached the empty-interval rule)."""
    plant = np.array(plant, float)
    rows = np.asarray(rows, float)
    heat = np.asarray(heat, int)
    B = plant.shape[0]
    hl, hw = float(half_length), float(half_width)
    k = R.new_carry(B) if carry is None else {a: np.array(b) for a, b in carry.items()}
    kk = new_carry(B) if ccarry is None else {a: np.array(b) for a, b in ccarry.items()}
    part = participants(plant, heat, nstep)
    out = dict(shelter=np.full(B, np.nan), mu=np.full(B, np.nan), impulse=np.full(B, np.nan), impulse_total=np.full(B, np.nan),
               leader=np.full(B, -1), hit=np.zeros(B, int), hit_ticks=np.zeros(B, int), first_hit_tick=np.full(B, -1), draft_ticks=np.zeros(B, int),
               friction_impulse=np.full(B, np.nan), yaw_kick=np.full(B, np.nan), yaw_kick_total=np.full(B, np.nan),
               partners=np.zeros(B, int), max_partners=np.zeros(B, int))
    member = heat >= 0
    for name in ("shelter", "impulse", "friction_impulse", "yaw_kick"):
        out[name][member] = 0.0
    out["mu"][member] = rows[member, 6]
    mu_live = rows[:, 6].copy()
    new = plant.copy()
    written = np.zeros(B, bool)
    margin = clip_margin = np.inf
    empties = 0
    gain, WL, WH = float(cfg["draft_gain"]), float(cfg["wake_length"]), float(cfg["wake_half_width"])
    for g in sorted(set(heat[member].tolist())):
        veh = np.nonzero((heat == g) & part)[0]                            # ascending: the member order
        n = veh.shape[0]
        if n == 0:
            continue
        P = plant[veh]
        x, y, vx, vy, yaw = P[:, 0], P[:, 1], P[:, 2], P[:, 3], P[:, 6]
        c, s = np.cos(yaw), np.sin(yaw)
        ux, uy = c * vx - s * vy, s * vx + c * vy
        mu = rows[veh, 6]
        wake, over, mg = R._decide(P, cfg, hl, hw)
        margin = min(margin, mg)
        dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
        lon = -(dx * c[None, :] + dy * s[None, :])
        alat = np.abs(-dx * s[None, :] + dy * c[None, :])
        w = np.where(wake, (1.0 - lon / WL) * (1.0 - alat / WH), 0.0)
        pairs = {}
        if cfg["contact"]:
            for i in range(n):
                for j in np.nonzero(over[i])[0]:
                    if i < j:
                        margin = min(margin, R._axis_margin(P[i, [0, 1, 6]], P[j, [0, 1, 6]], hl, hw))
                        r64, dec = respond(P[i], P[j], rows[veh[i], 2], rows[veh[i], 3], rows[veh[j], 2], rows[veh[j], 3], cfg, ccfg, hl, hw)
                        assert r64 is not None, "the overlap decision and the pair's own disagree"
                        margin = min(margin, dec["hard"]); clip_margin = min(clip_margin, dec["soft"]); empties += int(dec["empty"])
                        pairs[(i, int(j))] = r64
        for i in range(n):
            b = veh[i]
            best = float(w[i].max()) if n > 1 else 0.0
            lead = -1
            if best > 0:
                lead = int(veh[int(np.argmax(w[i]))])
                rest = np.sort(w[i])[::-1]
                if n > 2 and rest[1] != rest[0]:
                    margin = min(margin, float(rest[0] - rest[1]))
            sdu, sdc, sdw, imp, fimp, kick, partners = [0.0, 0.0], [0.0, 0.0], 0.0, 0.0, 0.0, 0.0, 0
            if cfg["contact"]:
                for j in np.nonzero(over[i])[0]:                           # ascending partners
                    r = pairs[(min(i, int(j)), max(i, int(j)))]
                    side = "a" if i < j else "b"
                    du, dw, dc = r["du_" + side], r["dw_" + side], r["dc_" + side]
                    sdu = [sdu[0] + du[0], sdu[1] + du[1]]; sdc = [sdc[0] + dc[0], sdc[1] + dc[1]]; sdw = sdw + dw
                    imp = imp + abs(r["Jn"]); fimp = fimp + abs(r["Jt"]); kick = kick + abs(dw); partners += 1
            hit = int(partners > 0)
            mu_live[b] = mu[i] * (1.0 - gain * best)
            if hit:
                un = (ux[i] + sdu[0], uy[i] + sdu[1])
                new[b, 2] = max(c[i] * un[0] + s[i] * un[1], 0.0)
                new[b, 3] = -s[i] * un[0] + c[i] * un[1]
                new[b, 0] = x[i] + sdc[0]; new[b, 1] = y[i] + sdc[1]
                if ccfg["yaw_response"]:
                    new[b, 7] = P[i, 7] + sdw
                written[b] = True
            out["shelter"][b] = best; out["mu"][b] = mu_live[b]; out["impulse"][b] = imp; out["leader"][b] = lead; out["hit"][b] = hit
            out["friction_impulse"][b] = fimp; out["yaw_kick"][b] = sdw; out["partners"][b] = partners
            k["impulse_total"][b] += imp; k["hit_ticks"][b] += hit; k["draft_ticks"][b] += int(best > 0)
            if hit and k["first_hit_tick"][b] < 0:
                k["first_hit_tick"][b] = t
            kk["yaw_kick_total"][b] += kick; kk["max_partners"][b] = max(kk["max_partners"][b], partners)
    for name in ("impulse_total", "hit_ticks", "first_hit_tick", "draft_ticks"):
        out[name][member] = k[name][member]
    for name in ("yaw_kick_total", "max_partners"):
        out[name][member] = kk[name][member]
    out.update(plant=new, mu_live=mu_live, carry=k, ccarry=kk, written=written, part=part, margin=float(margin),
               clip_margin=float(clip_margin), empty=empties)
    return out


def energy(plant, rows, sel):
    """Kinetic energy of the vehicles sel, rotation included."""
    P = np.asarray(plant, float)[sel]
    r = np.asarray(rows, float)[sel]
    return float(np.sum(0.5 * r[:, 2] * (P[:, 2] ** 2 + P[:, 3] ** 2) + 0.5 * r[:, 3] * P[:, 7] ** 2))


def angular_momentum(plant, rows, sel, at):
    """sum m (c x u) + Iz w of the vehicles sel about the origin, the centres taken from ``at``, and the tolerance's scale
    sum m |c| |u| + Iz |w|."""
    P, A = np.asarray(plant, float)[sel], np.asarray(at, float)[sel]
    r = np.asarray(rows, float)[sel]
    c, s = np.cos(P[:, 6]), np.sin(P[:, 6])
    ux, uy = c * P[:, 2] - s * P[:, 3], s * P[:, 2] + c * P[:, 3]
    L = np.sum(r[:, 2] * (A[:, 0] * uy - A[:, 1] * ux) + r[:, 3] * P[:, 7])
    scale = np.sum(r[:, 2] * (np.abs(A[:, 0]) + np.abs(A[:, 1])) * (np.abs(ux) + np.abs(uy)) + r[:, 3] * np.abs(P[:, 7]))
    return float(L), float(scale)


def contact_race_ref():
    """The class of the host replay of a race with the interactions and the contact model attached."""
    from tests import _tyre_ref as T

    class ContactRaceRef(R.interacting_race_ref()):
        """InteractingRaceRef whose tick is this module's: psiDot is handed to the simulator steps as well."""

        def __init__(self, track, plant0, heat, inter_cfg, contact_cfg, **kw):
            super().__init__(track, plant0, heat, inter_cfg, **kw)
            self.contact_cfg = contact_cfg
            self.contact_carry = new_carry(self.B)
            self.clip_margin = np.inf
            self.empty = 0

        def tick(self):
            self.inter = None
            if self.t >= self.attach_tick:
                steps = ((self.phase < 2) & np.isfinite(self.plant).all(axis=1)).astype(int)
                self.inter = tick(self.plant.copy(), np.array(self.rows), self.heat, self.inter_cfg, self.contact_cfg, t=self.t, nstep=steps,
                                  carry=self.inter_carry, ccarry=self.contact_carry, half_length=self.extents[0], half_width=self.extents[1])
                self.inter_carry, self.contact_carry = self.inter["carry"], self.inter["ccarry"]
                self.margin = min(self.margin, self.inter["margin"])
                self.clip_margin = min(self.clip_margin, self.inter["clip_margin"])
                self.empty += self.inter["empty"]
                self._advanced = np.zeros(self.B, bool)
            T.TyreRaceRef.tick(self)
            if self.inter is not None and np.any(self.inter["part"] & ~self._advanced):
                raise RuntimeError("tick %d: vehicles %s were counted as participants and did not advance" %
                                   (self.t - 1, np.nonzero(self.inter["part"] & ~self._advanced)[0].tolist()))

        def _advance(self, b, st, n):
            if self.inter is not None and self.inter["part"][b] and self.inter["written"][b]:
                st = st.copy()
                st[7] = self.inter["plant"][b, 7]
            return super()._advance(b, st, n)

    return ContactRaceRef
