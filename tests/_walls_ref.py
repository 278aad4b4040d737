"""Numpy restatement of the walls (include/lpvmpc.h, "Walls"), written from the header, not from the kernel.

Two parts, as tests/_interactions_ref.py.  The DECISIONS -- which rows see and accept a point, which accepted row is the nearest, which
corners penetrate, which corner is the deepest, whether the corner approaches the wall (vn against 0), whether the friction impulse is
clamped, whether the centre is located -- are evaluated in numpy.longdouble, and ``margin`` is the smallest distance of any of them from
its threshold: a scene whose margin is at least 1e-6 is decided alike by any float64 evaluation.  ``margins`` names the smallest margin of
each kind.  The VALUES are float64 with the header's operation order, every product and sum rounded on its own."""
import numpy as np

LD = np.longdouble
PI = 3.14159265358979323846           # the float64 pi of the row arithmetic

F64_NAMES = ("depth", "impulse", "impulse_total", "max_impulse")
I32_NAMES = ("hit", "side", "corner", "hit_ticks", "first_hit_tick", "outside")
DEFAULTS = dict(margin=0.25, reach=0.5, half_length=0.4, half_width_car=0.2, restitution=0.2, friction=0.3, push=0.5, yaw_response=1)
CORNER_SIGNS = ((1, 1), (1, -1), (-1, 1), (-1, -1))
KINDS = ("sees", "accepts", "row", "depth", "deepest", "vn", "clamp")


def config(**words):
    c = dict(DEFAULTS)
    c.update(words)
    return c


def new_carry(B):
    return dict(impulse_total=np.zeros(B), max_impulse=np.zeros(B), hit_ticks=np.zeros(B, int), first_hit_tick=np.full(B, -1, int))


def participants(plant, nstep=None):
    plant = np.asarray(plant, float)
    ns = np.ones(plant.shape[0], int) if nstep is None else np.asarray(nstep, int)
    return (ns > 0) & np.isfinite(plant[:, [0, 1, 6, 2, 3, 7]]).all(axis=1)


def _angle(ax, ay, ox, oy, bx, by):
    """computeAngle(a, o, b) in the type of its arguments."""
    v1x, v1y, v2x, v2y = ax - ox, ay - oy, bx - ox, by - oy
    return np.arctan2(v1x * v2y - v1y * v2x, v1x * v2x + v1y * v2y)


def _norm(dx, dy):
    return np.sqrt(dx * dx + dy * dy)


def row_locate(T, i, x, y, ty=float):
    """Row i of table T for the point (x, y), evaluated in type ty: (sees, ey, th, m_sees) -- m_sees the distance of the row's "sees"
    decision from its threshold (inf where an exact coincidence decides)."""
    rows = T.shape[0]
    ip = i - 1 if i > 0 else rows - 1
    c = lambda v: ty(v)
    x, y = c(x), c(y)
    xf, yf, xs, ys, ang, cv = c(T[i, 0]), c(T[i, 1]), c(T[ip, 0]), c(T[ip, 1]), c(T[ip, 2]), c(T[i, 5])
    half = c(PI) / 2
    at_s, at_f = _norm(xs - x, ys - y) == 0, _norm(xf - x, yf - y) == 0
    if cv == 0:
        if at_s or at_f:
            return True, c(0.0), ang, np.inf
        a1, a2 = abs(_angle(x, y, xs, ys, xf, yf)), abs(_angle(x, y, xf, yf, xs, ys))
        sees = bool(a1 <= half and a2 <= half)
        n1 = _norm(x - xs, y - ys)
        a = _angle(xf, yf, xs, ys, x, y)
        m = min(abs(a1 - half), abs(a2 - half)) if sees else max(a1 - half, a2 - half)
        return sees, n1 * np.sin(a), ang, float(m)
    if at_s:
        return True, c(0.0), ang, np.inf
    if at_f:
        return True, c(0.0), c(T[i, 2]), np.inf
    r = 1 / cv
    d = c(1.0) if r >= 0 else c(-1.0)
    cx, cy = xs + abs(r) * np.cos(ang + d * c(PI) / 2), ys + abs(r) * np.sin(ang + d * c(PI) / 2)
    arc1 = c(T[i, 4]) * cv
    arc2 = _angle(xs, ys, cx, cy, x, y)
    sees = bool(np.sign(arc1) == np.sign(arc2) and abs(arc1) >= abs(arc2))
    # the distance to the nearer end of the arc's sector: arc2 against 0 and against arc1
    m = min(abs(arc2), abs(abs(arc1) - abs(arc2))) if np.sign(arc1) == np.sign(arc2) else abs(arc2)
    return sees, -d * (_norm(x - cx, y - cy) - abs(r)), ang + arc2, float(m)


def locate(T, x, y, bound, note):
    """The search over all rows for the point (x, y): (located, ey, th) in float64 with the header's arithmetic; the decisions are taken
    in long double and their margins go to note(kind, margin)."""
    best, out = None, (False, 0.0, 0.0)
    cand = []
    for i in range(T.shape[0]):
        sees_l, ey_l, _, m_sees = row_locate(T, i, x, y, LD)
        if abs(ey_l) <= LD(bound) + LD(1e-3):                              # a row that could not accept the point anyway decides nothing
            note("sees", m_sees)
        if not sees_l:
            continue
        note("accepts", float(abs(abs(ey_l) - LD(bound))))
        if abs(ey_l) > LD(bound):
            continue
        cand.append(float(abs(ey_l)))
        _, ey, th, _ = row_locate(T, i, x, y, float)
        if best is None or abs(ey_l) < best:
            best, out = abs(ey_l), (True, float(ey), float(th))
    if len(cand) > 1:
        c = sorted(cand)
        note("row", c[1] - c[0])
    return out


def corners(plant, cfg):
    p = np.asarray(plant, float)
    c, s = np.cos(p[:, 6]), np.sin(p[:, 6])
    r = np.empty((p.shape[0], 4, 2))
    for k, (sa, sb) in enumerate(CORNER_SIGNS):
        a, b = sa * float(cfg["half_length"]), sb * float(cfg["half_width_car"])
        r[:, k, 0] = c * a - s * b
        r[:, k, 1] = s * a + c * b
    return r, p[:, None, [0, 1]] + r


def respond(st, row, r, n, depth, cfg, note=lambda k, m: None):
    """The response at the contact corner: st [8] before -> st after, and |Jn|.  r the corner's arm, n the inward normal."""
    e, f, push = float(cfg["restitution"]), float(cfg["friction"]), float(cfg["push"])
    x, y, vx, vy, yaw, w = st[0], st[1], st[2], st[3], st[6], st[7]
    m, Iz = float(row[2]), float(row[3])
    c, s = np.cos(yaw), np.sin(yaw)
    ux, uy = c * vx - s * vy, s * vx + c * vy
    rx, ry = (float(r[0]), float(r[1])) if cfg["yaw_response"] else (0.0, 0.0)
    nx, ny = float(n[0]), float(n[1])
    tx, ty = -ny, nx
    vcx, vcy = ux + w * -ry, uy + w * rx
    vn = vcx * nx + vcy * ny
    note("vn", abs(vn))
    rn = rx * ny - ry * nx
    kn = 1.0 / m + (rn * rn) / Iz
    Jn = (-(1.0 + e) * vn) / kn if vn < 0 else 0.0
    qn = Jn / m
    ux1, uy1, w1 = ux + qn * nx, uy + qn * ny, w + (rn * Jn) / Iz
    vdx, vdy = ux1 + w1 * -ry, uy1 + w1 * rx
    vt = vdx * tx + vdy * ty
    rt = rx * ty - ry * tx
    kt = 1.0 / m + (rt * rt) / Iz
    lim = f * Jn
    Jt = -vt / kt
    if Jn > 0:
        note("clamp", abs(abs(Jt) - lim))
    if Jt > lim:
        Jt = lim
    if Jt < -lim:
        Jt = -lim
    qt = Jt / m
    ux2, uy2, w2 = ux1 + qt * tx, uy1 + qt * ty, w1 + (rt * Jt) / Iz
    new = np.array(st, float)
    new[2] = max(c * ux2 + s * uy2, 0.0)
    new[3] = -s * ux2 + c * uy2
    if cfg["yaw_response"]:
        new[7] = w2
    k2 = push * depth
    new[0] = x + k2 * nx; new[1] = y + k2 * ny
    return new, abs(Jn), dict(vn=vn, Jn=Jn, Jt=Jt, u=(ux, uy), u2=(ux2, uy2), w2=w2 if cfg["yaw_response"] else w, r=(rx, ry))


def tick(plant, rows, track, half_width, cfg, t=0, nstep=None, carry=None, track_of=None):
    """One tick.  plant [B, 8], rows [B, 7] plant rows, track one table [rows, 6] or, with track_of [B], a list of tables, half_width
    one value or one per table.  Returns a dict: plant (after), the named outputs, carry, written [B], part [B], margin and margins."""
    plant = np.array(plant, float)
    rows = np.asarray(rows, float)
    B = plant.shape[0]
    k = new_carry(B) if carry is None else {a: np.array(b) for a, b in carry.items()}
    part = participants(plant, nstep)
    out = dict(depth=np.zeros(B), impulse=np.zeros(B), hit=np.zeros(B, int), side=np.zeros(B, int), corner=np.full(B, -1),
               outside=np.zeros(B, int))
    margins = {kind: np.inf for kind in KINDS}

    def note(kind, m):
        margins[kind] = min(margins[kind], float(m))
    new = plant.copy()
    written = np.zeros(B, bool)
    detail = [None] * B
    arms, pts = corners(plant, cfg)
    for b in np.nonzero(part)[0]:
        T = np.asarray(track if track_of is None else track[track_of[b]], float)
        hw = float(half_width if track_of is None else half_width[track_of[b]])
        wall_ey = hw + float(cfg["margin"])
        bound = wall_ey + float(cfg["reach"])
        found = [locate(T, pts[b, q, 0], pts[b, q, 1], bound, note) for q in range(4)]
        depth = np.zeros(4)
        for q, (ok, ey, _) in enumerate(found):
            if ok:
                note("depth", abs(abs(ey) - wall_ey))
                if abs(ey) > wall_ey:
                    depth[q] = abs(ey) - wall_ey
        out["outside"][b] = int(not locate(T, plant[b, 0], plant[b, 1], bound, note)[0])
        if depth.max() > 0:
            q = int(np.argmax(depth))                                      # the first that attains the max
            others = np.delete(depth, q)
            note("deepest", depth[q] - others.max())
            _, ey, th = found[q]
            sd = 1.0 if ey > 0 else -1.0
            n = (sd * np.sin(th), -(sd * np.cos(th)))
            new[b], imp, detail[b] = respond(plant[b], rows[b], arms[b, q], n, depth[q], cfg, note)
            detail[b].update(n=n, depth=depth[q])
            written[b] = True
            out["depth"][b] = depth[q]; out["impulse"][b] = imp; out["hit"][b] = 1; out["side"][b] = int(sd); out["corner"][b] = q
            k["impulse_total"][b] += imp; k["max_impulse"][b] = max(k["max_impulse"][b], imp); k["hit_ticks"][b] += 1
            if k["first_hit_tick"][b] < 0:
                k["first_hit_tick"][b] = t
    for name in ("impulse_total", "max_impulse", "hit_ticks", "first_hit_tick"):
        out[name] = k[name].copy()
    out.update(plant=new, carry=k, written=written, part=part, margin=min(margins.values()), margins=margins, detail=detail)
    return out


def kinetic_energy(st, row):
    """m |u|^2 / 2 + Iz w^2 / 2 of one plant row (|u| is the body-frame speed: a rotation keeps it)."""
    return 0.5 * row[2] * (st[2] * st[2] + st[3] * st[3]) + 0.5 * row[3] * st[7] * st[7]


def walled_race_ref():
    """The class of the host replay of a race with walls attached (imported lazily: the replay needs the oracle's solver)."""
    from tests import _tyre_ref as T

    class WalledRaceRef(T.TyreRaceRef):
        """TyreRaceRef with the walls ``wall_cfg`` attached from tick attach_tick on (None: never) and, optionally, the disturbances'
        kicks ``kicks`` [B, 3] = (kick_step, kick_vy, kick_w) (the other disturbance words off).  tick() computes the walls' tick from
        all plants at its top, the kick of this tick applied first as on the device (the disturbances' kernel runs in front of the
        walls'); _advance hands vehicle b that state in front of its simulator steps.  Lap 0 only: it raises when a vehicle it counted
        as a participant does not advance on that tick, or leaves lap 0."""

        def __init__(self, track, plant0, wall_cfg, kicks=None, attach_tick=0, **kw):
            T.TyreRaceRef.__init__(self, track, plant0, **kw)
            self.wall_cfg, self.wall_attach = wall_cfg, attach_tick
            self.kicks = None if kicks is None else np.asarray(kicks, float)
            self.wall_carry = new_carry(self.B)
            self.wall = None
            self.margin = np.inf

        def tick(self):
            if np.any(self.phase == 1):
                raise RuntimeError("WalledRaceRef replays lap 0 only")
            steps = ((self.phase < 2) & np.isfinite(self.plant).all(axis=1)).astype(int)
            self._pre = self.plant.copy()
            if self.kicks is not None:
                for b in np.nonzero(steps)[0]:
                    k0 = self.act[b].k
                    if k0 <= self.kicks[b, 0] < k0 + self.n_sub_lap0:
                        self._pre[b, 3] = self._pre[b, 3] + self.kicks[b, 1]; self._pre[b, 7] = self._pre[b, 7] + self.kicks[b, 2]
            self.wall = None
            self._advanced = np.zeros(self.B, bool)
            if self.wall_cfg is not None and self.t >= self.wall_attach:
                self.wall = tick(self._pre, np.array(self.rows), self.track, self.hw, self.wall_cfg, t=self.t, nstep=steps, carry=self.wall_carry)
                self.wall_carry = self.wall["carry"]
                self.margin = min(self.margin, self.wall["margin"])
            T.TyreRaceRef.tick(self)
            if self.wall is not None and np.any(self.wall["part"] & ~self._advanced):
                raise RuntimeError("tick %d: vehicles %s were counted as participants and did not advance" %
                                   (self.t - 1, np.nonzero(self.wall["part"] & ~self._advanced)[0].tolist()))

        def _advance(self, b, st, n):
            assert n == self.n_sub_lap0
            self._advanced[b] = True
            st = self._pre[b].copy()
            if self.wall is not None and self.wall["written"][b]:
                st = self.wall["plant"][b].copy()
            return T.TyreRaceRef._advance(self, b, st, n)

    return WalledRaceRef
