"""Scenes for the driver-policy tests (tests/test_driver_policy.py): small batches as plain arrays, in the format of
driver_scenes.py.

open_loop(E)   eight scenarios of width E, each built around one policy driver D and two other entities X, Y (the only three slots at
               E == 3; at larger widths they sit on slots that straddle the 64-slot blocks, and the other slots hold fillers far from
               every corridor, every fifth of them not in the scene).  Everybody stands still, so the reset state holds the poses
               exactly as written here.  Scenario by scenario:
                 0  two candidates with bit-equal gap (X, Y; X is a caller-run driver, so policy positions differ from list positions)
                 1  X beside the driver with a negative gap; Y not in the scene, inside the corridor; a path of one point
                 2  X exactly at gap == REACH; Y one ulp of its own coordinate outside the corridor on the left, nearer than X
                 3  X one ulp beyond REACH; Y as much outside the corridor on the right
                 4  off-axis box centres for driver and lead, the lead (Y, in another 64-block from E = 65 on) rotated by 90 degrees,
                    the driver facing against its path of 65 points
                 5  D equidistant from two segments of a path with zero-length segments in the middle and at its end; X, a second
                    policy driver, nearest to a zero-length segment at the start of its path; Y a plain lead
                 6  REACH = +inf with a lead 500 m ahead, a path of 130 points; X a policy driver that has not spawned, with a path
                    of no points
                 7  a driver that reverses (allow_reverse; its speed is negative after the PRE steps of pre_actions)
column(n)      n scenarios: a slow replay car followed by four policy drivers on a gently curved path that ends inside the scene.
mixed()        the column with two caller-run drivers beside it.
"""
import numpy as np

DT = 0.1
CAR = (2.0, 4.0, 1.0, 0.0)  # width, length, center_x, center_y: front = 3 m ahead of the pose point
KIND_REPLAY, KIND_AGENT_REPLAY, KIND_AGENT_EXTERNAL = 1, 2, 6
DEFAULT_CTRL = np.array([0.7, 5.0, np.nan, 0.0, 0.03054, 1.5709, 0.3753, 1.8970, 0.0204, 0.0, 5.0, 0.0, 1.0, 0, 0, 0])
LENGTH = 10.0
PRE = 3  # steps of sg_step_drivers ahead of the second open-loop comparison
(V0, T, S0, A, B, HALF, REACH, K_PSI, K_E, K_SOFT, GAP_MIN) = range(11)
NPARAM = 12


def params(v0=10.0, T=1.5, s0=2.0, a=1.5, b=2.0, half=0.25, reach=80.0, k_psi=1.0, k_e=0.5, k_soft=1.0, gap_min=0.1):
    row = np.zeros(NPARAM)
    row[:11] = (v0, T, s0, a, b, half, reach, k_psi, k_e, k_soft, gap_min)
    return row


def _still(x, y, h, t0=0.0, t1=LENGTH):
    """Two knots at one place: in the scene from t0 to t1."""
    k = np.zeros((2, 7))
    k[:, 0] = (t0, t1)
    k[:, 1], k[:, 2], k[:, 4] = x, y, h
    return k


def _along(pts, speed, t0=0.0):
    """Knots on the polyline pts at constant speed, heading along each segment."""
    pts = np.asarray(pts, np.float64)
    seg = np.diff(pts, axis=0)
    s = np.concatenate([[0.0], np.cumsum(np.hypot(seg[:, 0], seg[:, 1]))])
    h = np.arctan2(seg[:, 1], seg[:, 0])
    k = np.zeros((len(pts), 7))
    k[:, 0] = t0 + s / speed
    k[:, 1:3] = pts
    k[:, 4] = np.concatenate([h, h[-1:]])
    return k


def _scenario(E, r, ents):
    """ents: {slot: dict(knots, bbox=CAR, driver=False, ctrl=(max_steer, max_accel, max_speed, allow_reverse))}; the other slots
    are fillers.  The ego is the first slot that is no driver and in the scene from the start (slot 0 when there is none)."""
    knots, bbox, kind, ctrl = [], np.tile(np.array(CAR), (E, 1)), np.full(E, KIND_REPLAY, np.int32), np.tile(DEFAULT_CTRL, (E, 1))
    for i in range(E):
        e = ents.get(i)
        if e is None:
            late = i % 5 == 4
            knots.append(_still(1000.0 + 20.0 * i, 1000.0 + 50.0 * r, 0.3 * i, 5.0 if late else 0.0))
            continue
        knots.append(e["knots"])
        bbox[i] = e.get("bbox", CAR)
        if e.get("driver"):
            kind[i] = KIND_AGENT_EXTERNAL
            ctrl[i, :4] = e.get("ctrl", (0.7, 5.0, np.nan, 0.0))
    plain = [i for i in range(E) if kind[i] != KIND_AGENT_EXTERNAL and knots[i][0, 0] <= 0.0]  # (in the scene from the start)
    ego = plain[0] if plain else 0
    if plain:
        kind[ego] = KIND_AGENT_REPLAY
    off = np.concatenate([[0], np.cumsum([len(k) for k in knots])]).astype(np.int64)
    return dict(knot_off=off, knots=np.concatenate(knots), bbox=bbox, etype=np.zeros(E, np.int32), ego=int(ego), t0=0.0, length=LENGTH,
                kind=kind, ctrl=ctrl, drivers=sorted(i for i in ents if ents[i].get("driver")))


def pack(scs):
    from scenario_gym_amd.packing import pack_arrays

    return pack_arrays(scs, kinds=[s["kind"] for s in scs], ctrls=[s["ctrl"] for s in scs])


def driver_list(scs):
    scen = [r for r, s in enumerate(scs) for _ in s["drivers"]]
    slot = [k for s in scs for k in s["drivers"]]
    return np.array(scen, np.int32), np.array(slot, np.int32)


def slots_of(E, r):
    """(D, X, Y) of scenario r: the only three slots at E == 3, else slots at the ends of the 64-slot blocks."""
    if E == 3:
        return tuple((r + q) % 3 for q in range(3))
    return (0, min(63, E - 2), E - 1) if r % 2 == 0 else (E - 1, 0, E // 2)


def arc(x, y, h, radius, n, step):
    """n points from (x, y) along a circle of `radius` (to the left) that starts with heading h, `step` apart."""
    a = h + np.arange(n) * step / radius
    return np.stack([x + radius * (np.sin(a) - np.sin(h)), y - radius * (np.cos(a) - np.cos(h))], 1)


UP = float(np.nextafter(2.25, 3.0))  # lat - hw = 1.25 + one ulp for a 2 m wide box: just outside a corridor of HALF = 0.25
P5 = np.array([(-10.0, 0.0), (0.0, 0.0), (0.0, 0.0), (0.0, 10.0), (0.0, 10.0)])  # zero-length segments 1 (middle) and 3 (end)


def open_loop(E):
    """dict(scs, scen, slot: the driver list; driver: the policy's positions in it; params [m, 12]; paths; who: (scenario, role) of every
    policy driver; nominal_v: its speed in the hand-made state of the CPU test; pre_actions [PRE, n_drivers, 2])."""
    scs, pol = [], []  # pol: (scenario, slot, role, parameter row, path, nominal speed)

    def drv(knots, **kw):
        return dict(knots=knots, driver=True, **kw)

    def add(r, ents):
        scs.append(_scenario(E, r, ents))

    d, x, y = slots_of(E, 0)
    add(0, {d: drv(_still(0.0, 0.0, 0.0)), x: drv(_still(20.0, 0.5, 0.0)), y: dict(knots=_still(20.0, -0.5, 0.0))})
    pol.append((0, d, "tie", params(), np.array([(0.0, 0.0), (100.0, 0.0)]), 0.0))
    d, x, y = slots_of(E, 1)
    add(1, {d: drv(_still(0.0, 0.0, 0.0)), x: dict(knots=_still(1.0, 1.5, 0.0)), y: dict(knots=_still(0.5, 0.0, 0.0, 5.0))})
    pol.append((1, d, "beside", params(), np.array([(0.0, 0.0)]), 0.0))
    d, x, y = slots_of(E, 2)
    add(2, {d: drv(_still(0.0, 0.0, 0.0)), x: dict(knots=_still(20.0, 0.0, 0.0)), y: dict(knots=_still(10.0, UP, 0.0))})
    pol.append((2, d, "reach", params(reach=16.0), np.array([(-5.0, -1.0), (50.0, 3.0)]), 0.0))
    d, x, y = slots_of(E, 3)
    add(3, {d: drv(_still(0.0, 0.0, 0.0)), x: dict(knots=_still(float(np.nextafter(20.0, 21.0)), 0.0, 0.0)), y: dict(knots=_still(10.0, -UP, 0.0))})
    pol.append((3, d, "beyond", params(reach=16.0), np.array([(-5.0, 1.0), (50.0, -3.0)]), 0.0))
    d, x, y = slots_of(E, 4)
    h = 1.1
    ahead = lambda q: (3.0 + q * np.cos(h), -7.0 + q * np.sin(h))  # noqa: E731
    add(4, {d: drv(_still(3.0, -7.0, h), bbox=(2.0, 4.0, 1.5, 0.5)), x: dict(knots=_still(*ahead(30.0), h)),
            y: dict(knots=_still(*ahead(15.0), h + 0.5 * np.pi), bbox=(2.0, 4.5, 0.75, -0.25))})
    pol.append((4, d, "against", params(), arc(*ahead(40.0), h + np.pi, 500.0, 65, 1.0), 0.0))
    d, x, y = slots_of(E, 5)
    add(5, {d: drv(_still(-5.0, 5.0, 0.4)), x: drv(_still(97.0, 0.0, 0.2)), y: dict(knots=_still(-5.0 + 12.0 * np.cos(0.4), 5.0 + 12.0 * np.sin(0.4), 0.4))})
    pol.append((5, d, "equidistant", params(), P5, 0.0))
    pol.append((5, x, "zero_first", params(), np.array([(100.0, 0.0), (100.0, 0.0), (110.0, 0.0)]), 0.0))
    d, x, y = slots_of(E, 6)
    add(6, {d: drv(_still(0.0, 0.0, 0.05)), x: drv(_still(30.0, 2.0, 0.0, 5.0)), y: dict(knots=_still(500.0 * np.cos(0.05), 500.0 * np.sin(0.05), 0.05))})
    pol.append((6, d, "far", params(reach=np.inf), arc(-20.0, -1.0, 0.05, 300.0, 130, 2.0), 0.0))
    pol.append((6, x, "unspawned", params(), np.zeros((0, 2)), 0.0))
    d, x, y = slots_of(E, 7)
    add(7, {d: drv(_still(0.0, 0.0, -0.3), ctrl=(0.7, 5.0, np.nan, 1.0)), x: dict(knots=_still(11.0 * np.cos(-0.3), 11.0 * np.sin(-0.3), -0.3)),
            y: dict(knots=_still(40.0, 40.0, 0.0))})
    pol.append((7, d, "reverse", params(), np.array([(-10.0, 3.0), (60.0, -19.0)]), -0.5 * PRE))

    scen, slot = driver_list(scs)
    pos = {(int(r), int(k)): i for i, (r, k) in enumerate(zip(scen, slot))}
    pol.sort(key=lambda q: pos[(q[0], q[1])])
    pre = np.zeros((PRE, len(scen), 2))
    pre[:, pos[(7, slots_of(E, 7)[0])]] = (-9.0, 0.3)  # (beyond max_accel: -5 m/s^2 for PRE steps)
    return dict(scs=scs, scen=scen, slot=slot, driver=np.array([pos[(q[0], q[1])] for q in pol], np.int64), params=np.array([q[3] for q in pol]),
                paths=[q[4] for q in pol], who=[(q[0], q[2]) for q in pol], nominal_v=np.array([q[5] for q in pol]), pre_actions=pre)


# ---- the closed-loop scenes ----------------------------------------------------------------------------------------------------
STEPS = 60
N_FOLLOW = 4
LEAD_SPEED = 4.0
SPEED_MARGIN = 0.5  # every follower ends within this of the lead's speed (m/s)
COLUMN_E = 8        # slots 0..4: the lead and its followers; 5, 6: the caller-run drivers of mixed(); 7: a filler
PATH = arc(0.0, 0.0, 0.0, 400.0, 74, 1.0)  # 73 m of a 400 m circle: it ends inside the scene
SPACING, V_START = 12.0, 4.3               # pose to pose, and the followers' speed at the start, in scenario 0


def column(n=2, mixed=False):
    """n scenarios.  Slot 0: the lead, a replay car at LEAD_SPEED along the circle of PATH and on beyond its end; slots 1..4: the
    followers, policy drivers on PATH, follower j starting (j * spacing) m behind the lead at its own speed.  mixed: slots 5 and 6
    are caller-run drivers on a parallel road 30 m to the right.  dict as open_loop() gives it, with follow: (scenario, slot) of
    every follower and lead_slot."""
    scs, pol = [], []
    for r in range(n):
        spacing, v = SPACING + 0.5 * r, V_START + 0.2 * r
        s_lead = 50.0  # the lead's arclength at t = 0
        at = lambda s: (400.0 * np.sin(s / 400.0), 400.0 * (1.0 - np.cos(s / 400.0)), s / 400.0)  # noqa: E731
        ents = {0: dict(knots=_along(arc(*at(s_lead), 400.0, 40, 2.0), LEAD_SPEED))}
        for j in range(1, N_FOLLOW + 1):
            x, y, h = at(s_lead - j * spacing)
            k = _still(x, y, h)
            k[1, 1:3] = x + v * LENGTH * np.cos(h), y + v * LENGTH * np.sin(h)  # (a recording at speed v: the reset's controller speed)
            ents[j] = dict(knots=k, driver=True)
            pol.append((r, j, "follower", params(v0=8.0), PATH, v))
        if mixed:
            for q, slot in enumerate((5, 6)):
                k = _still(10.0 + 25.0 * q, -30.0, 0.0)
                k[1, 1] += 5.0 * LENGTH
                ents[slot] = dict(knots=k, driver=True)
        scs.append(_scenario(COLUMN_E, r, ents))
    scen, slot = driver_list(scs)
    pos = {(int(r), int(k)): i for i, (r, k) in enumerate(zip(scen, slot))}
    pol.sort(key=lambda q: pos[(q[0], q[1])])
    return dict(scs=scs, scen=scen, slot=slot, driver=np.array([pos[(q[0], q[1])] for q in pol], np.int64), params=np.array([q[3] for q in pol]),
                paths=[q[4] for q in pol], who=[(q[0], q[2]) for q in pol], nominal_v=np.array([q[5] for q in pol]),
                follow=[(q[0], q[1]) for q in pol], lead_slot=0)


def cut_at(sc, length):
    """The scenario with every recording ending at `length`: its knots before that time and the interpolated pose there."""
    out = []
    for e in range(len(sc["etype"])):
        k = sc["knots"][sc["knot_off"][e]:sc["knot_off"][e + 1]]
        n = int((k[:, 0] < length).sum())
        assert 0 < n < len(k)
        last = k[n - 1] + (k[n] - k[n - 1]) * ((length - k[n - 1, 0]) / (k[n, 0] - k[n - 1, 0]))
        last[0] = length
        out.append(np.concatenate([k[:n], last[None]]))
    off = np.concatenate([[0], np.cumsum([len(k) for k in out])]).astype(np.int64)
    return dict(sc, knot_off=off, knots=np.concatenate(out), length=float(length))


def caller_actions(n_drivers, policy_positions, seed=0):
    """[STEPS, n_drivers, 2] random (accel, steer) for the caller-run drivers; the policy's rows hold a pattern that must never reach
    a controller (99 m/s^2, full lock)."""
    rng = np.random.default_rng([20251019, seed, n_drivers])
    a = np.empty((STEPS, n_drivers, 2))
    a[..., 0] = rng.uniform(-2.0, 2.0, (STEPS, n_drivers))
    a[..., 1] = rng.uniform(-0.2, 0.2, (STEPS, n_drivers))
    a[:, policy_positions] = (99.0, 1.5)
    return a
