"""Inputs of the heats' GPU tests (tests/test_gpu_heats.py), shared with the host test that holds them to their conditions
(tests/test_heats_host.py): no pair of the crafted geometry lies inside the band of tests/_heats_ref.py except the two pairs placed
exactly touching on purpose (TOUCHING), and every scripted sequence contains a pass, a wrap, a hold, a finish and a loss."""
import numpy as np

HL, HW = 0.4, 0.2           # the default footprint


def crafted():
    """One tick, B = 80: three heats with interleaved membership (sizes 1, 5 and 65: one more than a wavefront), nine vehicles in no
    heat.  Returns a dict of the heat_step arguments, `touching` (the two pairs placed exactly touching, by vehicle index) and
    `named` (vehicle indices of the named poses)."""
    B = 80
    heat = np.full(B, -1, int)
    free = [b for b in range(B) if b % 8 != 7 or b > 71]                # nine vehicles (7, 15, .., 71) stay in no heat
    assert len(free) == 71
    for i, b in enumerate(free):
        heat[b] = 0 if i == 10 else 1 if i in (3, 17, 30, 44, 60) else 2
    big = np.nonzero(heat == 2)[0]
    assert big.shape[0] == 65 and np.sum(heat == 1) == 5 and np.sum(heat == 0) == 1
    P = []
    names = {}

    def put(name, *poses):
        names[name] = [int(big[len(P) + k]) for k in range(len(poses))]
        P.extend(poses)

    put("side_by_side", (0.0, 0.0, 0.0), (0.0, 0.53, 0.0))                            # gap 0.53 - 0.4 = 0.13
    put("nose_to_tail", (10.0, 0.0, 0.0), (10.85, 0.0, 0.0))                          # gap 0.05
    put("t_bone", (20.0, 0.0, 0.0), (20.57, 0.0, np.pi / 2))                          # overlap 0.03
    put("corners_45", (30.0, 0.0, 0.0), (30.0 + 0.4 + 0.45, 0.2 + 0.45, np.pi / 4))
    put("identical", (40.0, 0.0, 0.3), (40.0, 0.0, 0.3), (40.0, 0.0, 0.3))
    put("touching_nose", (50.0, 0.0, 0.0), (50.8, 0.0, 0.0))
    put("touching_side", (60.0, 0.0, 0.0), (60.0, 0.4, 0.0))
    put("far", (1000.0, 1000.0, 1.0))
    put("nan_pose", (np.nan, 5.0, 0.0))
    k = 0
    while len(P) < 65:                                          # a line of cars 3 m apart and more (no two neighbours equally far), yaw turning
        P.append((3.0 * k + 0.1 * k * k, 100.0, 0.37 * k)); k += 1
    pose = np.zeros((B, 3))
    pose[big] = np.array(P)
    small = np.nonzero(heat == 1)[0]
    pose[small] = [(0.9 * i, 50.0 + 0.05 * i, 0.15 * i * i - 0.3) for i in range(5)]       # five cars in a row, some overlapping
    pose[heat == 0] = (5.0, 5.0, 2.0)
    pose[heat < 0] = (7.0, 7.0, 0.0)                                                   # ignored
    rng = np.random.default_rng(11)
    L = np.full(B, 18.7)
    s = np.round(rng.uniform(0.0, 18.7, B), 3)
    s[big[20:26]] = s[big[20]]                                                          # equal progress: the index breaks the tie
    inside = np.ones(B, int)
    inside[big[30:34]] = 0; s[big[30:34]] = 10000.0                                     # never located: class 2
    inside[names["nan_pose"][0]] = 0; s[names["nan_pose"][0]] = 10000.0
    phase = np.where(np.arange(B) % 2, 1, 0)
    phase[big[40:44]] = 2; phase[big[44:47]] = 3                                        # finished (two of them before the attach), lost
    phase[small[4]] = 2
    phase0 = np.zeros(B, int); phase0[big[40:42]] = 2
    turns0 = np.zeros(B, int); turns0[big[50:55]] = [-1, 1, 2, -1, 3]
    touching = [tuple(names["touching_nose"]), tuple(names["touching_side"])]
    return dict(heat=heat, L=L, pose=pose, s=s, inside=inside, phase=phase, phase0=phase0, turns0=turns0, touching=touching, named=names,
                hl=HL, hw=HW)


def crafted_256():
    """One heat of exactly 256 on a 16 x 16 grid with jittered poses, some cars overlapping; every class present."""
    B = 256
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    pose = np.stack([0.9 * gx.ravel() + rng.uniform(-0.2, 0.2, B), 0.6 * gy.ravel() + rng.uniform(-0.1, 0.1, B), rng.uniform(-3.1, 3.1, B)], axis=1)
    L = np.full(B, 31.4)
    s = np.round(rng.uniform(0.0, 31.4, B), 2)
    inside = (rng.uniform(size=B) > 0.1).astype(int)
    s[inside == 0] = 10000.0
    phase = rng.choice([0, 1, 1, 1, 2, 3], B)
    return dict(heat=np.zeros(B, int), L=L, pose=pose, s=s, inside=inside, phase=phase, phase0=np.zeros(B, int),
                turns0=rng.integers(-1, 2, B), touching=[], named={}, hl=HL, hw=HW)


SEQ_HL, SEQ_HW = 0.5, 0.25      # dyadic extents: with yaw 0 and dyadic positions every sep of a sequence is exact in float64
SEQ_TICKS = 12


def sequence(scale):
    """A scripted sequence of 12 ticks for B = 8 (heat 0: vehicles 0 1 2 4 5 7; heat 1: vehicle 3; vehicle 6 in none) on a track of
    L = 16 * scale, every distance scaled alike.  It holds: an overtake (1 passes 0 on tick 5) and a re-pass (0 passes 1 on tick
    9), forward wraps with line crossings (0 on tick 8, 1 on tick 7; 7 starts at turns0 = -1 and crosses on tick 8), a backward wrap
    (2 on tick 3), a car off the track for ticks 3 .. 5 and held (4; 5 passes it on tick 4 and is re-passed on tick 6), a finisher
    on tick 9 (5) and a second on tick 11 (1), and a loss on tick 10 (7).  Returns (static, ticks): static = heat, L, turns0; ticks a
    list of dicts pose, s, inside, phase."""
    c = float(scale)
    Lt = 16.0 * c
    heat = np.array([0, 0, 0, 1, 0, 0, -1, 0])
    turns0 = np.array([0, 0, 0, 0, 0, 0, 0, -1])
    ticks = []
    for t in range(SEQ_TICKS):
        u = np.zeros(8)                                                 # unwrapped distance along the track, in units of `scale`
        u[0] = 12 + 0.5 * t
        u[1] = 11 + 0.75 * t if t <= 7 else 16.25 + 0.125 * (t - 7)
        u[2] = 0.5 - 0.25 * t if t <= 5 else -0.75 + 0.5 * (t - 5)
        u[3] = 1.0 + t
        u[4] = 5 + 0.5 * t
        u[5] = 4.5 + 0.5 * min(t, 9)
        u[6] = 3.0
        u[7] = 14 + 0.25 * t
        if t >= 11:
            u[1] = 16.25 + 0.125 * 4                                    # frozen once finished
        s = np.mod(u, 16.0) * c
        inside = np.ones(8, int)
        phase = np.ones(8, int)
        lane = np.array([0.0, 0.0, 1.0, 0.0, 2.0, 2.5, 9.0, 4.0])       # 0 and 1 share a lane, 4 and 5 overlap across theirs
        pose = np.stack([u * c, lane * c, np.zeros(8)], axis=1)
        if t < 2:
            inside[3] = 0; s[3] = 10000.0                               # 3 is not located before tick 2: class 2
        if 3 <= t <= 5:
            inside[4] = 0; s[4] = 10000.0                               # 4 is off the track and held
            if t == 4:
                pose[4, 0] = np.nan                                     # ... on one tick without a pose: no partner of anyone
        if t >= 9:
            phase[5] = 2
        if t >= 11:
            phase[1] = 2
        if t >= 10:
            phase[7] = 3; inside[7] = 0; s[7] = 10000.0; pose[7] = np.nan
        ticks.append(dict(pose=pose, s=s, inside=inside, phase=phase))
    return dict(heat=heat, L=np.full(8, Lt), turns0=turns0), ticks


SEQUENCES = {"unit": 1.0, "double": 2.0}
