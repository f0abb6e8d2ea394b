"""Scenes for the route-observation tests (tests/test_routes.py): small batches as plain arrays, built with the helpers of
policy_scenes.py (imported as they are).

batch(E)   four scenarios of width E.  Twelve roles, three per scenario, on slots that sit at the ends of the 64-slot blocks (the only
           three slots at E == 3); the other slots are the fillers of policy_scenes._scenario, far away, every fifth not in the scene.
             r0, r1, r2, r3, r64, r65, r66, r130   an entity with a route of that many points.  r65 stands beside segment 63 of its
                        route (the last lane of the first block of 64), r66 beside segment 64 (alone in the second block), r130 beside
                        segment 100; r2 and r130 are replay cars that move, the others drivers that start at rest
             late       a driver whose recording starts at t = 5: not in the scene at the reset; the first step spawns it, and it
                        is then in the scene before its first knot
             short      a driver whose recording ends at t = 0.45: ten steps later it is in the scene after its last knot
             single     a replay entity with one knot at t = 0: in the scene at the reset alone
             none       a driver without a route
           The observer list: every role, one filler per 64-slot block (in the scene, no route), a filler that is not in the scene,
           the ego of every scenario, and the first two observers once more.
hand()     the hand-made scenes of the CPU tests: poses and routes with exact answers.
"""
import numpy as np

import policy_scenes as PS

ROLES = ("r0", "r1", "r2", "r3", "r64", "r65", "r66", "r130", "late", "short", "single", "none")
N_POINTS = dict(r0=0, r1=1, r2=2, r3=3, r64=64, r65=65, r66=66, r130=130)
BESIDE = dict(r64=30, r65=63, r66=64, r130=100)  # the segment the entity stands beside
STEPS = 10


def spots(E):
    """Slots at the ends of the 64-slot blocks of a scenario of width E."""
    return sorted({s for s in (0, 1, 2, 63, 64, 65, 127, 128, 300, 511, 512, 575, E - 1) if 0 <= s < E})


def slots_of(E, r):
    """The three role slots of scenario r."""
    sp = spots(E)
    n = len(sp)
    step = (n + 2) // 3
    return [sp[(r + j * step) % n] for j in range(3)]


def _beside(path, j, side):
    """A point `side` metres to the left of the middle of segment j of path, and the segment's direction."""
    a, b = path[j], path[j + 1]
    e = b - a
    ln = np.hypot(e[0], e[1])
    mid = 0.5 * (a + b)
    return mid[0] - side * e[1] / ln, mid[1] + side * e[0] / ln, float(np.arctan2(e[1], e[0]))


def batch(E):
    """dict(scs, who: {role: (scenario, slot)}, routes: {(scenario, slot): path}, drv_scen, drv_slot: the driver list, obs_scen,
    obs_slot: the observer list, actions [STEPS, n_drivers, 2])."""
    ents = [dict() for _ in range(4)]
    who, routes = {}, {}
    for k, role in enumerate(ROLES):
        r, j = k % 4, k // 4
        slot = slots_of(E, r)[j]
        who[role] = (r, slot)
        x0, y0, h = 150.0 * k, -40.0 * k, 0.3 + 0.35 * k
        path = None
        if role in N_POINTS:
            path = PS.arc(x0, y0, h, 120.0 + 10.0 * k, N_POINTS[role], 1.5)
        if role in BESIDE:
            x, y, hh = _beside(path, BESIDE[role], 1.25)
            knots = PS._still(x, y, hh + 0.2)
        elif role in ("r2", "r130"):
            knots = PS._along([(x0, y0 + 2.0), (x0 + 20.0 * np.cos(h), y0 + 2.0 + 20.0 * np.sin(h))], 5.0)
        else:
            knots = PS._still(x0 + 1.0, y0 - 0.75, h - 0.1)
        if role == "r130":  # a replay car beside segment 100, moving along it
            x, y, hh = _beside(path, BESIDE[role], -0.75)
            knots = PS._along([(x, y), (x + 20.0 * np.cos(hh), y + 20.0 * np.sin(hh))], 5.0)
        if role == "late":
            knots = PS._still(x0, y0, h, 5.0)
            path = np.array([(x0 - 5.0, y0 - 1.0), (x0 + 5.0, y0 + 1.0), (x0 + 9.0, y0 + 6.0)])
        if role == "short":
            knots = PS._still(x0, y0, h, 0.0, 0.45)
            knots[1, 1:3] = x0 + 2.0 * np.cos(h), y0 + 2.0 * np.sin(h)
            path = knots[:, 1:3].copy()
        if role == "single":
            knots = PS._still(x0, y0, h)[:1]
            path = np.array([(x0 - 3.0, y0 - 4.0), (x0 + 9.0, y0 + 1.0)])
        driver = role not in ("r2", "r130", "single")
        ents[r][slot] = dict(knots=knots, driver=driver)
        if path is not None:
            routes[(r, slot)] = np.asarray(path, np.float64).reshape(-1, 2)
    scs = [PS._scenario(E, r, ents[r]) for r in range(4)]
    drv_scen, drv_slot = PS.driver_list(scs)
    obs = [who[role] for role in ROLES]
    special = {(r, s) for r in range(4) for s in ents[r]}
    for b in range((E + 63) // 64):  # a filler of every block that is in the scene (slot % 5 != 4), and one that is not
        for r in (b % 4,):
            cand = [s for s in range(64 * b, min(64 * b + 64, E)) if (r, s) not in special and s % 5 != 4]
            if cand:
                obs.append((r, cand[len(cand) // 2]))
    absent = [(r, s) for r in range(4) for s in range(E) if (r, s) not in special and s % 5 == 4]
    obs += absent[:1]
    obs += [(r, scs[r]["ego"]) for r in range(4)]
    obs += obs[:2]
    rng = np.random.default_rng([20261019, E])
    actions = np.empty((STEPS, len(drv_scen), 2))
    actions[..., 0] = rng.uniform(1.0, 3.0, actions.shape[:2])
    actions[..., 1] = rng.uniform(0.05, 0.3, actions.shape[:2]) * np.where(rng.random(actions.shape[:2]) < 0.5, -1.0, 1.0)
    return dict(scs=scs, who=who, routes=routes, drv_scen=drv_scen, drv_slot=drv_slot, obs_scen=np.array([r for r, _ in obs], np.int32),
                obs_slot=np.array([s for _, s in obs], np.int32), actions=actions)


def route_lists(routes):
    """(scenario, slot, paths) of a routes dict, in its order."""
    return np.array([r for r, _ in routes], np.int32), np.array([s for _, s in routes], np.int32), list(routes.values())


def hand():
    """The hand-made scenes: {name: dict(pose (x, y, h), path, n_ahead, spacing)}; one observer each, in the scene, on a
    recording of two knots at its pose."""
    axis = np.array([(0.0, 0.0), (10.0, 0.0), (20.0, 0.0)])
    return dict(
        offset345=dict(pose=(13.0, 4.0, 0.0), path=np.array([(0.0, 0.0), (10.0, 0.0)]), n_ahead=0, spacing=0.0),  # 3 beyond the end, 4 beside: 5 away
        left4=dict(pose=(4.0, 4.0, 0.0), path=axis, n_ahead=2, spacing=3.0),
        vertex=dict(pose=(10.0, 0.0, 0.0), path=np.array([(0.0, 0.0), (10.0, 0.0), (10.0, 10.0)]), n_ahead=0, spacing=0.0),
        shared=dict(pose=(12.0, -2.0, 0.0), path=np.array([(0.0, 0.0), (10.0, 0.0), (10.0, 10.0)]), n_ahead=0, spacing=0.0),
        zero_len=dict(pose=(6.0, 1.0, 0.0), path=np.array([(0.0, 0.0), (4.0, 0.0), (4.0, 0.0), (12.0, 0.0), (12.0, 0.0)]), n_ahead=4, spacing=2.0),
        on_cum=dict(pose=(2.0, 1.0, 0.0), path=np.array([(0.0, 0.0), (4.0, 0.0), (4.0, 8.0)]), n_ahead=5, spacing=2.0),  # targets 4 (a cum), 6, ..., 12 (total)
        beyond=dict(pose=(8.0, -1.0, 0.0), path=axis, n_ahead=3, spacing=8.0),
        against=dict(pose=(5.0, 0.5, np.pi), path=axis, n_ahead=1, spacing=2.0),
    )
