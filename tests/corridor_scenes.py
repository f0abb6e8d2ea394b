"""Scenes for the tests of the driver policy's corridor along the path (tests/test_policy_corridor.py): small batches in the format
of policy_scenes.py, whose helpers build them.

open_loop(E)   scenarios of width E, each built around one policy driver D and two other entities X, Y on the slots of
               policy_scenes.slots_of (the only three slots at E == 3; at larger widths they straddle the 64-slot blocks, the other
               slots hold fillers far from every corridor, every fifth of them not in the scene).  Everybody stands still, so the reset
               state holds the poses exactly as written here.  A car is policy_scenes.CAR: 2 m wide, 4 m long, its centre 1 m ahead
               of its pose point, so front = 3, hl = 2 and hw = 1 along a segment.  The straight paths run along +x from the origin
               with vertices at dyadic coordinates, so arclengths and gaps are exact.  Every driver has CORRIDOR == 1 unless said.
                 0  bend          20 m straight, then a left arc of radius 30 m through 90 degrees in 5 degree segments; X on the arc
                                  40 degrees round it, Y straight ahead of D, 9 m outside the arc
                 1  mixed         the bend again with two policy drivers: X (CORRIDOR == 0) stands behind D (CORRIDOR == 1), Y on the arc
                 2  tie           X (a caller-run driver) and Y with bit-equal gap 16; zero-length segments inside the window
                 3  reach         X exactly at gap == REACH; Y one ulp outside `left`, nearer than X
                 4  beyond        X one ulp beyond REACH; Y one ulp outside `right`
                 5  window_in     the second segment starts exactly at the window bound: X is measured on it
                 6  window_out    the same with that segment starting one ulp later: X is measured on the first segment's end
                 7  equidistant   X equidistant from the two segments of a 90 degree corner (inside it): the lower index; Y in the
                                  corner's outer wedge, outside the `res` limit
                 8  wedge         X in the outer wedge inside the `res` limit (the lead); Y outside it, nearer if admitted
                 9  zero_best     D's own best segment is a zero-length segment at the start of its path; X beside D has that
                                  segment as its best one (a tie with the next, the lower index) and is refused; Y a plain lead
                10  path_end      a path of 2 points; X beyond its end and in line with it, refused by `res`; Y beyond the end within
                                  the limit, the lead
                11  off_path      D half a metre left of its path; Y inside the corridor only if `off` were forgotten; X the lead
                12  against       D faces against its path: X, behind its back but ahead along the path, is the lead; Y, before its
                                  bonnet, is the straight rule's
                13  negative_front D's box lies behind its pose point (front = -6) and REACH = 4: the window is empty; X would be a
                                  candidate of a window that held the first segment, and is one of the straight rule
                14  crossing      a path that crosses itself; D on the later pass; X beside the earlier pass (an index below g), Y ahead
                15  presence      Y inside the corridor and nearer, not in the scene; X the lead, a policy driver that has spawned; the
                                  scenario's second policy driver sits in scenario 16
                16  fallback      CORRIDOR == 1 with a path of one point: the straight rule; X a policy driver that has not spawned
                17  rotated       a path of 65 points (an arc); D and Y with off-axis box centres, Y rotated by 90 degrees against the
                                  path; X further along
                18  overlap       a path of 130 points, D at its vertex 80 (g beyond index 64); X beside D with a negative gap; Y ahead
column(n)      n scenarios on the bend, its straight part drawn out backwards: a slow replay car on the arc followed by four policy
               drivers with CORRIDOR == 1.
"""
import numpy as np

import policy_scenes as PS

CORRIDOR = 11  # SG_DP_CORRIDOR
UP = PS.UP     # 2.25 + one ulp


def params(corridor=1.0, **kw):
    row = PS.params(**kw)
    row[CORRIDOR] = corridor
    return row


def bend_path(back=0.0, step=10.0):
    """From (-back, 0) along +x to (20, 0) (vertices `step` apart behind the origin), then a left arc of radius 30 m about (20, 30)
    through 90 degrees, a vertex every 5 degrees."""
    xs = [-back + step * i for i in range(int(round(back / step)))] + [0.0, 20.0]
    a = np.deg2rad(np.arange(5.0, 90.5, 5.0))
    return np.concatenate([np.stack([xs, np.zeros(len(xs))], 1), np.stack([20.0 + 30.0 * np.sin(a), 30.0 - 30.0 * np.cos(a)], 1)])


def on_arc(deg):
    """The pose (x, y, heading) on the bend's arc `deg` degrees round it."""
    a = float(np.deg2rad(deg))
    return 20.0 + 30.0 * np.sin(a), 30.0 - 30.0 * np.cos(a), a


STRAIGHT = np.array([(0.0, 0.0), (16.0, 0.0), (32.0, 0.0), (64.0, 0.0), (128.0, 0.0)])
WITH_ZEROS = np.array([(0.0, 0.0), (16.0, 0.0), (16.0, 0.0), (32.0, 0.0), (32.0, 0.0), (64.0, 0.0)])
CORNER = np.array([(0.0, 0.0), (16.0, 0.0), (16.0, 32.0)])
CROSSING = np.array([(8.0, -16.0), (8.0, 16.0), (-16.0, 16.0), (-16.0, 0.0), (0.0, 0.0), (16.0, 0.0), (32.0, 0.0)])
ARC65 = PS.arc(0.0, 0.0, 0.3, 100.0, 65, 1.0)
ARC130 = PS.arc(-20.0, -1.0, 0.05, 300.0, 130, 2.0)
LONG = (2.0, 5.0, 1.0, 0.0)  # a longer box: hl = 2.5


def _at(path_fn_args, i, lateral=0.0, turn=0.0):
    """The pose at vertex i of an arc of policy_scenes.arc(x, y, h, radius, n, step), `lateral` metres to its left, turned by `turn`."""
    x, y, h, radius, _, step = path_fn_args
    a = h + i * step / radius
    px, py = x + radius * (np.sin(a) - np.sin(h)), y - radius * (np.cos(a) - np.cos(h))
    return float(px - lateral * np.sin(a)), float(py + lateral * np.cos(a)), float(a + turn)


A65 = (0.0, 0.0, 0.3, 100.0, 65, 1.0)
A130 = (-20.0, -1.0, 0.05, 300.0, 130, 2.0)


def open_loop(E):
    """dict(scs, scen, slot: the driver list; driver: the policy's positions in it; params [m, 12]; paths; who: (scenario, role) of every
    policy driver; nominal_v; pre_actions [PRE, n_drivers, 2]), as policy_scenes.open_loop gives it."""
    scs, pol = [], []
    still = PS._still

    def drv(knots, **kw):
        return dict(knots=knots, driver=True, **kw)

    def car(x, y, h=0.0, **kw):
        return dict(knots=still(x, y, h), **kw)

    def add(role, ents, path, prm=None, d_slot=None):
        r = len(scs)
        scs.append(PS._scenario(E, r, ents))
        pol.append((r, PS.slots_of(E, r)[0] if d_slot is None else d_slot, role, params() if prm is None else prm, np.asarray(path, np.float64), 0.0))

    S = lambda: PS.slots_of(E, len(scs))  # noqa: E731
    d, x, y = S()
    add("bend", {d: drv(still(5.0, 0.0, 0.0)), x: car(*on_arc(40.0)), y: car(45.0, 0.0)}, bend_path())
    d, x, y = S()
    add("mixed", {d: drv(still(5.0, 0.0, 0.0)), x: drv(still(-7.0, 0.0, 0.0)), y: car(*on_arc(40.0))}, bend_path())
    pol.append((1, x, "mixed_straight", params(corridor=0.0), bend_path(), 0.0))
    d, x, y = S()
    add("tie", {d: drv(still(0.0, 0.0, 0.0)), x: drv(still(20.0, 0.5, 0.0)), y: car(20.0, -0.5)}, WITH_ZEROS)
    d, x, y = S()
    add("reach", {d: drv(still(0.0, 0.0, 0.0)), x: car(20.0, 0.0), y: car(10.0, UP)}, STRAIGHT, params(reach=16.0))
    d, x, y = S()
    add("beyond", {d: drv(still(0.0, 0.0, 0.0)), x: car(float(np.nextafter(20.0, 21.0)), 0.0), y: car(10.0, -UP)}, STRAIGHT, params(reach=16.0))
    d, x, y = S()
    add("window_in", {d: drv(still(0.0, 0.0, 0.0)), x: car(16.0, 0.0), y: car(40.0, 40.0)}, [(0.0, 0.0), (16.0, 0.0), (32.0, 0.0)], params(reach=13.0))
    d, x, y = S()
    add("window_out", {d: drv(still(0.0, 0.0, 0.0)), x: car(16.0, 0.0), y: car(40.0, 40.0)},
        [(0.0, 0.0), (float(np.nextafter(16.0, 17.0)), 0.0), (32.0, 0.0)], params(reach=13.0))
    d, x, y = S()
    add("equidistant", {d: drv(still(0.0, 0.0, 0.0)), x: car(11.0, 4.0), y: car(18.0, -0.5, bbox=LONG)}, CORNER, params(half=4.0))
    d, x, y = S()
    add("wedge", {d: drv(still(0.0, 0.0, 0.0)), x: car(16.0, -0.5), y: car(18.0, -0.5, bbox=LONG)}, CORNER)
    d, x, y = S()
    add("zero_best", {d: drv(still(0.0, 0.0, 0.0), bbox=(2.0, 2.0, 0.0, 0.0)), x: car(-1.0, 1.5), y: car(20.0, 0.0)},
        [(0.0, 0.0), (0.0, 0.0), (16.0, 0.0), (32.0, 0.0)])
    d, x, y = S()
    add("path_end", {d: drv(still(0.0, 0.0, 0.0)), x: car(19.0, 0.0, bbox=LONG), y: car(16.5, 0.0)}, [(0.0, 0.0), (16.0, 0.0)])
    d, x, y = S()
    add("off_path", {d: drv(still(0.0, 0.5, 0.0)), x: car(20.0, 1.0), y: car(10.0, -1.8)}, STRAIGHT)
    d, x, y = S()
    add("against", {d: drv(still(50.0, 0.0, np.pi)), x: car(70.0, 0.0), y: car(30.0, 0.0, np.pi)}, STRAIGHT)
    d, x, y = S()
    add("negative_front", {d: drv(still(0.0, 0.0, 0.0), bbox=(2.0, 4.0, -8.0, 0.0)), x: car(-2.0, 0.0), y: car(40.0, 40.0)},
        [(0.0, 0.0), (16.0, 0.0)], params(reach=4.0))
    d, x, y = S()
    add("crossing", {d: drv(still(-8.0, 0.0, 0.0)), x: car(8.0, 5.0, 0.5 * np.pi), y: car(20.0, 0.0)}, CROSSING)
    d, x, y = S()
    add("presence", {d: drv(still(0.0, 0.0, 0.0)), x: drv(still(20.0, 0.0, 0.0)), y: dict(knots=still(8.0, 0.0, 0.0, 5.0))}, STRAIGHT)
    pol.append((15, x, "spawned", params(), STRAIGHT, 0.0))
    d, x, y = S()
    add("fallback", {d: drv(still(0.0, 0.0, 0.2)), x: drv(still(30.0, 2.0, 0.0, 5.0)), y: car(20.0 * np.cos(0.2), 20.0 * np.sin(0.2), 0.2)}, [(1.0, 1.0)])
    pol.append((16, x, "unspawned", params(), STRAIGHT, 0.0))
    d, x, y = S()
    add("rotated", {d: drv(still(*_at(A65, 10)), bbox=(2.0, 4.0, 1.5, 0.5)), x: car(*_at(A65, 45)),
                    y: car(*_at(A65, 30, turn=0.5 * np.pi), bbox=(2.0, 4.5, 0.75, -0.25))}, ARC65)
    d, x, y = S()
    add("overlap", {d: drv(still(*_at(A130, 80))), x: car(*_at(A130, 80.5, lateral=-1.7)), y: car(*_at(A130, 90))}, ARC130)

    scen, slot = PS.driver_list(scs)
    pos = {(int(r), int(k)): i for i, (r, k) in enumerate(zip(scen, slot))}
    pol.sort(key=lambda q: pos[(q[0], q[1])])
    pre = np.zeros((PS.PRE, len(scen), 2))
    pre[:, [pos[(q[0], q[1])] for q in pol if q[2] in ("bend", "rotated", "overlap")]] = (1.5, 0.1)  # (three of them drive off)
    return dict(scs=scs, scen=scen, slot=slot, driver=np.array([pos[(q[0], q[1])] for q in pol], np.int64), params=np.array([q[3] for q in pol]),
                paths=[q[4] for q in pol], who=[(q[0], q[2]) for q in pol], nominal_v=np.array([q[5] for q in pol]), pre_actions=pre)


# ---- the closed-loop scene -----------------------------------------------------------------------------------------------------
STEPS = 60
BACK = 60.0
COLUMN_PATH = bend_path(BACK)  # 80 m straight, then the arc: 127.1 m


def column(n=2):
    """n scenarios.  Slot 0: the lead, a replay car at policy_scenes.LEAD_SPEED from 5 degrees round the arc, on round it and straight
    on beyond its end; slots 1..4: the followers, policy drivers with CORRIDOR == 1 on COLUMN_PATH, follower j starting j * spacing m
    behind the lead on the straight part, at its own speed, recorded driving on along the path.  dict as policy_scenes.column gives it."""
    scs, pol = [], []
    lead_pts = np.concatenate([COLUMN_PATH[-18:], [(50.0, 60.0), (50.0, 90.0)]])  # the arc's vertices from 5 degrees on, then +y
    s_lead = BACK + 20.0 + 30.0 * np.deg2rad(5.0)
    for r in range(n):
        spacing, v = PS.SPACING + 0.5 * r, PS.V_START + 0.2 * r
        ents = {0: dict(knots=PS._along(lead_pts, PS.LEAD_SPEED))}
        for j in range(1, PS.N_FOLLOW + 1):
            x = s_lead - j * spacing - BACK
            assert x < 20.0
            ahead = COLUMN_PATH[[i for i in range(len(COLUMN_PATH)) if i >= len(COLUMN_PATH) - 18 or COLUMN_PATH[i, 0] > x]]
            k = PS._along(np.concatenate([[(x, 0.0)], ahead]), v)  # (a recording along the path at speed v: the reset's controller speed)
            ents[j] = dict(knots=k, driver=True)
            pol.append((r, j, "follower", params(v0=8.0), COLUMN_PATH, v))
        scs.append(PS._scenario(PS.COLUMN_E, r, ents))
    scen, slot = PS.driver_list(scs)
    pos = {(int(r), int(k)): i for i, (r, k) in enumerate(zip(scen, slot))}
    pol.sort(key=lambda q: pos[(q[0], q[1])])
    return dict(scs=scs, scen=scen, slot=slot, driver=np.array([pos[(q[0], q[1])] for q in pol], np.int64), params=np.array([q[3] for q in pol]),
                paths=[q[4] for q in pol], who=[(q[0], q[2]) for q in pol], nominal_v=np.array([q[5] for q in pol]),
                follow=[(q[0], q[1]) for q in pol], lead_slot=0)
