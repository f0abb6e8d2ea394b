"""Scenes whose knot TIMES are the point: every entity on a clock of its own, knots on the engine's clock and one ulp beside it,
knots one ulp apart, union grids of thousands of rows, clocks that do not start at zero.  For the replay interpolant -- the
host's union grid (Upload::scenario, csrc/h_upload.hip), build_grid_kernel (sgym_grid.hpp), the segment cursor seg_locate /
seg_advance / seg_load (sgym_core.hpp) and its restatements in sgym_wide.hpp, sgym_control.hpp, sgym_rollout.hpp,
sgym_sensors.hpp and sgym_observers.hpp.  tests/test_knot_times_cpu.py, tests/test_gpu_knot_times.py and
tests/golden/make_golden_knots.py use it.  A plain module, like box_scenes.py: numpy only, seeded, deterministic, no import of
the engine.

Every other scene generator of the suite puts a scenario on ONE np.linspace grid, so the union grid is that grid, stage 1 of
the batch interpolant only reproduces knots, and the clock meets a grid row at t = 0 alone.  The families here:

  ragged   every entity its own sorted random times, 2 .. K knots: several union rows per step
  clock    knot times drawn from clock() itself: t == x[i] on most steps; a fifth of them one ulp down, a fifth one ulp up;
           first / last knots on clock values (entities enter and leave on the inclusive bound min_t <= t <= max_t); one-knot
           statics on a clock value (their second row at t + 0.1 is a row of the grid); in every other scenario the union
           grid begins one ulp above a clock value (the constant piece before the first row ends on the double below it)
  twins    knots from a pool of times shared by the scenario's entities, each taken as p, the ulp above, both, or the two ulps
           above: knots one ulp apart within an entity (with a jump of centimetres between them: the largest slopes), rows one
           ulp apart across entities; half the pool are clock values
  long     64 replay entities of 128 .. 256 knots: a union grid of more than 8,192 rows under fewer than 100 steps
  offset   the ego's first knot -- the start of the clock -- at 0.37, everybody else from negative times on

Poses are arcs (synthetic._chunk) in a yard small enough that boxes meet.  Each family has a static share, a share of late
spawns that vanish, and every other scenario carries z / pitch / roll (zpr="none": no scenario does, the planar kernels).
"""
import numpy as np

KIND_REPLAY, KIND_AGENT_REPLAY, KIND_AGENT_PID, KIND_AGENT_VEHICLE, KIND_AGENT_PEDESTRIAN = 1, 2, 3, 4, 5
C_PED_SPEED_DESIRED, C_PED_RADIUS = 9, 12
CAR = (2.0, 4.2, 1.37, 0.0)
PED_BOX = (0.69, 0.7, 0.0, 0.0)
FAMILIES = ("ragged", "clock", "twins", "long", "offset")
EGO_KIND = dict(replay=KIND_AGENT_REPLAY, pid=KIND_AGENT_PID, vehicle=KIND_AGENT_VEHICLE)
OFFSET_T0 = 0.37
FIRST = 3  # clock, odd scenarios: the clock value below the first row of the union grid
TAIL = 2  # clock values the recordings go on beyond the last step: no scenario ends (max_length) within its steps


def clock(t0, dt, n):
    """The engine's clock: n + 1 values, t[0] = t0, t[k + 1] = t[k] + dt in fp64 (NOT t0 + k * dt)."""
    t = np.empty(n + 1)
    t[0] = t0
    for k in range(n):
        t[k + 1] = t[k] + dt
    return t


def _up(t):
    return np.nextafter(t, np.inf)


def _down(t):
    return np.nextafter(t, -np.inf)


# ----------------------------------------------------------------------------------------------------------- knot times
def _random_times(rng, lo, hi, n):
    """n strictly increasing times, the first lo, the last hi."""
    while True:
        t = np.unique(np.concatenate([[lo, hi], rng.uniform(lo, hi, n - 2)]))
        if len(t) == n:
            return t


def _clock_times(rng, c, ia, ib, n, exact_ends):
    """n of the clock values c[ia .. ib] (both ends among them); a fifth one ulp down, a fifth one ulp up; exact_ends: the first
    and the last stay where they are."""
    n = min(n, ib - ia + 1)
    mid = ia + 1 + np.sort(rng.choice(ib - ia - 1, n - 2, replace=False)) if n > 2 else np.zeros(0, np.int64)
    t = c[np.concatenate([[ia], mid, [ib]]).astype(np.int64)]
    u = rng.random(n)
    if exact_ends:
        u[[0, -1]] = 0.5
    return np.where((u < 0.2) & (t != 0.0), _down(t), np.where(u > 0.8, _up(t), t))


def _twin_times(rng, pool, lo, hi, n, anchored):
    """(times, which of them are the upper knot of a pair one ulp apart): pool values of [lo, hi] (both ends among them), each
    as p / p and the ulp above / the ulp above / the two ulps above / the ulp below and p.  anchored: the first knot is lo."""
    inside = pool[(pool > lo) & (pool < hi)]
    m = min(max(n // 2, 2), len(inside) + 2)
    picks = np.concatenate([[lo], np.sort(rng.choice(inside, m - 2, replace=False)) if m > 2 else [], [hi]])
    t, upper = [], []
    for j, p in enumerate(picks):
        v = int(rng.integers(5))
        if p == 0.0 or (anchored and j == 0 and v in (2, 3, 4)):  # (the ulp of 0.0 is a denormal: no pair there)
            v = 0 if p == 0.0 else 1
        seq = ([p], [p, _up(p)], [_up(p)], [_up(p), _up(_up(p))], [_down(p), p])[v]
        t += seq
        upper += [False] + [True] * (len(seq) - 1)
    return np.array(t), np.array(upper)


# ----------------------------------------------------------------------------------------------------------- one scenario
def scene(family, E, r, ego="replay", dt=0.1, steps=40, K=10, zpr="half", crowd=False):
    """Scenario r of a family with E entities (plain arrays, as packing.pack_arrays takes them, + kind): ego "replay", "pid",
    "vehicle" or "sparse" (a PID ego in every fourth scenario, the others replay agents); K: most knots of an entity (long: 128 ..
    256 whatever K); crowd: four in ten of the others are pedestrian agents (routes, controller rows in "ped_ctrl")."""
    assert family in FAMILIES
    rng = np.random.default_rng([20251021, FAMILIES.index(family), E, r, K, int(round(1 / dt))])
    t0 = OFFSET_T0 if family == "offset" else 0.0
    c = clock(t0, dt, steps + TAIL)
    n_c = len(c) - 1
    side = np.sqrt((10.0 if not crowd else 6.0) * E) + 4.0
    p0 = rng.uniform(-side / 2, side / 2, (E, 2))
    h0 = rng.uniform(-np.pi, np.pi, E)
    v = rng.uniform(0.0, 8.0, E)
    kappa = rng.normal(0.0, 0.05, E)
    kappa = np.where(np.abs(kappa) < 1e-6, 1e-6, kappa)
    lift = (r % 2 == 1) and zpr == "half"
    u = rng.random(E)
    u[0] = 1.0  # the ego spans the run
    static = u < 0.15
    late = (~static) & (u < 0.4)  # late spawns that vanish
    if family == "long":
        static, late = u < 0.05, (u >= 0.05) & (u < 0.25)
    # clock, odd scenarios: nobody but the ego is there from the start, and the first to come has its first knot one ulp above
    # the clock value c[FIRST]: the union grid begins there, and the step to c[FIRST] ends on the double below its first row
    late_grid = family == "clock" and r % 2 == 1
    if late_grid:
        late = ~static
        late[0] = False
    first_ia = FIRST + 1 if late_grid else 1
    opened = not late_grid
    is_ped = np.zeros(E, bool)
    if crowd:
        is_ped[1:] = rng.random(E - 1) < 0.4
        is_ped[1] = True
    pool = np.unique(np.concatenate([c[[0, n_c]], c[rng.choice(n_c, min(3 * K, n_c) // 2, replace=False)], rng.uniform(c[0], c[-1], 3 * K // 2)]))
    kind = np.full(E, KIND_REPLAY, np.int32)
    kind[0] = EGO_KIND["pid" if r % 4 == 0 else "replay"] if ego == "sparse" else EGO_KIND[ego]
    kind[is_ped] = KIND_AGENT_PEDESTRIAN
    etype = np.where(is_ped, 1, 0).astype(np.int32)
    bbox = np.where(is_ped[:, None], np.array(PED_BOX), np.array(CAR))

    def pose(e, t, jump=None):
        h = h0[e] + kappa[e] * v[e] * t
        rows = np.zeros((len(t), 7))
        rows[:, 0] = t
        rows[:, 1] = p0[e, 0] + (np.sin(h) - np.sin(h0[e])) / kappa[e]
        rows[:, 2] = p0[e, 1] - (np.cos(h) - np.cos(h0[e])) / kappa[e]
        rows[:, 4] = h
        if lift:
            rows[:, 3], rows[:, 5], rows[:, 6] = 0.05 * v[e] * t, 0.02 * np.sin(0.7 * t + e), 0.01 * np.cos(0.9 * t + e)
        if jump is not None and jump.any():  # the upper knot of a pair one ulp apart: centimetres away from the lower one
            rows[jump, 1:3] += rng.normal(0.0, 0.02, (int(jump.sum()), 2))
            rows[jump, 4] += rng.normal(0.0, 1e-3, int(jump.sum()))
        return rows

    knots, off, routes, route_off = [], [0], [], [0]
    for e in range(E):
        jump = None
        if is_ped[e]:  # a pedestrian agent: its recording only places it
            t = c[[0, n_c]]
        elif static[e]:
            t = c[[int(rng.integers(first_ia if late_grid else 0, n_c))]] if family in ("clock", "twins") else rng.uniform(c[0], c[-1], 1)
        else:
            ia, ib = (int(rng.integers(first_ia, steps // 2)), int(rng.integers(steps // 2 + 1, steps))) if late[e] else (0, n_c)
            n = int(rng.integers(128, 257)) if family == "long" else int(rng.integers(2, K + 1))
            if family == "clock":
                opens = late[e] and not opened  # (the first late spawn of such a scenario opens the union grid)
                t = _clock_times(rng, c, FIRST if opens else ia, ib, n, exact_ends=e == 0 or opens or rng.random() < 0.75)
                if opens:
                    t[0], opened = _up(c[FIRST]), True
            elif family == "twins":
                t, jump = _twin_times(rng, pool, c[ia], c[ib], n, anchored=e == 0)
            else:
                lo, hi = c[ia] + (rng.uniform(0, dt) if late[e] else 0.0), c[ib] - (rng.uniform(0, dt) if late[e] else 0.0)
                if not late[e] and e > 0:
                    lo, hi = lo - (rng.uniform(0.0, 3.0) if family == "offset" else 0.0), hi + rng.uniform(0.0, 1.0)
                t = _random_times(rng, lo, hi, n)
        rows = pose(e, np.asarray(t, np.float64), jump)
        if is_ped[e]:
            rows[:, 1:3] = p0[e]
            rows[:, 4] = h0[e]
            routes.append(np.stack([p0[e], -p0[e] * rng.uniform(0.3, 1.0) + rng.normal(0.0, 2.0, 2)]))
        route_off.append(route_off[-1] + (2 if is_ped[e] else 0))
        knots.append(rows)
        off.append(off[-1] + len(rows))
    knots = np.concatenate(knots)
    off = np.array(off, np.int64)
    sc = dict(knot_off=off, knots=knots, bbox=bbox, etype=etype, kind=kind, ego=0, t0=float(max(0.0, knots[0, 0])),
              length=float(knots[off[1:] - 1, 0].max()), ctrl=None, family=family, dt=dt, steps=steps)
    assert sc["t0"] == t0 and sc["length"] >= c[-1]
    if crowd:
        sc["route_off"] = np.array(route_off, np.int64)
        sc["routes"] = np.concatenate(routes)
        sc["ped_ctrl"] = (is_ped, rng.uniform(0.5, 1.5, E) * 1.3, 3.0)
    return sc


_BATCHES = {}


def batch(family, E, R, ego="replay", dt=0.1, steps=40, K=10, zpr="half", crowd=False):
    """R scenarios of a family (cached: the CPU and the GPU tests share them)."""
    key = (family, E, R, ego, dt, steps, K, zpr, crowd)
    if key not in _BATCHES:
        _BATCHES[key] = [scene(family, E, r, ego, dt, steps, K, zpr, crowd) for r in range(R)]
    return _BATCHES[key]


def ctrl_rows(sc, default_ctrl):
    """[E][NCTRL] controller rows of a scenario: the defaults, and the pedestrian agents' desired speed and radius."""
    ctrl = np.tile(np.asarray(default_ctrl, np.float64), (len(sc["kind"]), 1))
    if "ped_ctrl" in sc:
        is_ped, vdes, rad = sc["ped_ctrl"]
        ctrl[is_ped, C_PED_SPEED_DESIRED] = vdes[is_ped]
        ctrl[is_ped, C_PED_RADIUS] = rad
    return ctrl


def replayed(sc):
    """(slots, knot_off, knots) of the entities of a scenario that go through the batch interpolant (kind REPLAY)."""
    slots = np.nonzero(np.asarray(sc["kind"]) == KIND_REPLAY)[0]
    off = np.asarray(sc["knot_off"])
    rows = [sc["knots"][off[e]:off[e + 1]] for e in slots]
    return slots, np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64), np.concatenate(rows)


# ----------------------------------------------------------------------------------------------------------- the reference
def _linear(x, y, xn):
    """interp1d(x, y, axis=0, bounds_error=False, fill_value=(y[0], y[-1]))(xn): _call_linear and the fill."""
    idx = np.clip(np.searchsorted(x, xn, side="left"), 1, len(x) - 1)
    lo, hi = idx - 1, idx
    slope = (y[hi] - y[lo]) / (x[hi] - x[lo])[:, None]
    out = slope * (xn - x[lo])[:, None] + y[lo]
    out[xn < x[0]] = y[0]
    out[xn > x[-1]] = y[-1]
    return out


def _datas(knot_off, knots):
    out = []
    for e in range(len(knot_off) - 1):
        d = np.nan_to_num(np.asarray(knots[knot_off[e]:knot_off[e + 1]], np.float64))
        if d.shape[0] == 1:
            d = np.repeat(d, 2, axis=0)
            d[-1, 0] += 1e-1
        out.append(d)
    return out


def union_grid(knot_off, knots):
    """The union grid of BatchReplayEntity.add_entities (one-knot entities bring their second row at t + 0.1)."""
    return np.unique(np.concatenate([d[:, 0] for d in _datas(knot_off, knots)]))


def batch_reference(knot_off, knots, q, persist=False):
    """BatchReplayEntity in numpy (add_entities with timestep None, then step's presence rule) at the times q:
    (poses [len(q)][E][6], present [len(q)][E])."""
    q = np.asarray(q, np.float64)
    datas = _datas(knot_off, knots)
    ts = np.unique(np.concatenate([d[:, 0] for d in datas]))
    X = np.concatenate([_linear(d[:, 0], d[:, 1:], ts) for d in datas], axis=1)  # stage 1: [N][E * 6]
    poses = _linear(ts, X, q).reshape(len(q), len(datas), 6)                       # stage 2
    n = np.diff(np.asarray(knot_off))
    lo, hi = knots[np.asarray(knot_off)[:-1], 0], knots[np.asarray(knot_off)[1:] - 1, 0]
    present = bool(persist) | (n == 1)[None, :] | ((q[:, None] >= lo[None, :]) & (q[:, None] <= hi[None, :]))
    return poses, present


def scipy_reference(knot_off, knots, q):
    """The two interp1d calls themselves (needs scipy): poses [len(q)][E][6]."""
    from scipy.interpolate import interp1d

    datas = _datas(knot_off, knots)
    ts = np.unique(np.concatenate([d[:, 0] for d in datas]))
    X = np.concatenate([interp1d(d[:, 0], d[:, 1:].T, bounds_error=False, fill_value=(d[0, 1:], d[-1, 1:]))(ts).T for d in datas], axis=1)
    return interp1d(ts, X.T, bounds_error=False, fill_value=(X[0], X[-1]))(np.asarray(q)).T.reshape(len(q), len(datas), 6)


# ----------------------------------------------------------------------------------------------------------- what a scene reaches
def coverage(sc, dt=None, steps=None):
    """Counts of what the replayed entities of a scene put in front of the interpolant over its steps (conditions on the
    INPUTS): steps whose next_t is a union row; (entity, step) pairs with next_t == the entity's first / last knot time (entities
    of several knots); union rows in total and per step; adjacent rows one ulp apart; entities that are in the scene at some
    step and not at another; steps whose next_t is the double below the first union row."""
    dt = sc["dt"] if dt is None else dt
    steps = sc["steps"] if steps is None else steps
    _, off, kn = replayed(sc)
    ts = union_grid(off, kn)
    t = clock(sc["t0"], dt, steps)[1:]
    many = np.diff(off) > 1
    lo, hi = kn[off[:-1], 0][many], kn[off[1:] - 1, 0][many]
    inside = (t[:, None] >= lo) & (t[:, None] <= hi)
    within = int(((ts > sc["t0"]) & (ts <= t[-1])).sum())
    return dict(on_row=int(np.isin(t, ts).sum()), on_min=int((t[:, None] == lo).sum()), on_max=int((t[:, None] == hi).sum()),
                rows=len(ts), rows_per_step=within / steps, ulp_pairs=int((_up(ts[:-1]) == ts[1:]).sum()),
                come_and_go=int((inside.any(0) & ~inside.all(0)).sum()), below_first=int((_up(t) == ts[0]).sum()), steps=steps)
