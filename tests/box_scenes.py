"""Scenes of MIXED bounding boxes for the collision pass and every other reader of a state block's box fields (ST_BW..ST_BCY:
rollout_body / tile_centre / the fp32 filter / REFINE in csrc/sgym_rollout.hpp and sgym_collide.hpp, wide_collide_kernel in
sgym_wide.hpp, the entity raster and the look-ahead in sgym_observers.hpp, classify_events_kernel and the RSS distances in
sgym_sensors.hpp), and the exact answer to "do these two boxes meet".  tests/test_boxes_cpu.py and tests/test_gpu_boxes.py use
it.  A plain module, like road_shapes.py: numpy only, seeded, deterministic; what needs the oracle takes its corners function
as an argument.

Box classes (width, length, center_x, center_y): a pedestrian-sized square, the car, a bus, an articulated lorry whose
reference point lies metres off its centre in BOTH components, "outside" boxes whose reference point is not in the box, skew
boxes with both centre components non-zero and of either sign, a zero-width and a zero-length box (segments: the reference
takes any extents and builds a polygon from the four corner points; the oracle's separating-axis test equals the exact
predicate on them, test_boxes_cpu.py).  Every yard scenario holds exactly one GIANT (a lorry or a bus, with a few small
boxes travelling beside its reference point): in the last occupied slot when the scenario has more than 64 slots --
another wavefront than the small boxes it meets, another 256-slot tile beyond 512 -- and in a random slot otherwise.
"""
from fractions import Fraction

import numpy as np

# SG_KIND_* (include/sgym.h) and the controller-row columns of the pedestrian agents
KIND_REPLAY, KIND_AGENT_REPLAY, KIND_AGENT_PID, KIND_AGENT_PEDESTRIAN = 1, 2, 3, 5
C_PED_SPEED_DESIRED, C_PED_RADIUS = 9, 12
DT = 0.1

PED_BOX = (0.5, 0.5, 0.0, 0.0)
CAR = (2.0, 4.2, 1.37, 0.0)
BUS = (2.55, 12.0, 4.1, -1.9)
LORRY = (2.6, 18.75, 6.0, 2.5)
OUTSIDE = ((1.8, 2.0, 3.0, 0.0), (1.8, 2.0, -3.0, 0.0), (1.0, 3.2, 0.4, 1.5), (1.0, 3.2, -0.4, -1.5))
SKEW = ((1.8, 4.6, 1.2, 0.45), (1.6, 3.8, -0.9, -0.5), (2.2, 6.0, 2.1, -0.7), (1.2, 2.4, -0.6, 0.8))
ZERO_EXTENT = ((0.0, 4.0, 1.0, 0.3), (2.0, 0.0, -0.5, 0.4))  # a zero-width and a zero-length box
SMALL = (PED_BOX, CAR) + OUTSIDE + SKEW + ZERO_EXTENT
SMALL_P = np.array([3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], float) / 16
EGO_BOXES = (CAR, SKEW[0], SKEW[2])  # (the controlled ego needs a length: the vehicle model steers by it)
GIANTS = (LORRY, BUS)

# scenarios per batch, by entity slots: the tile shapes of test_gpu_variants.SHAPES and two widths of the multi-kernel step
BATCH = {3: 16, 6: 12, 12: 8, 24: 6, 48: 4, 100: 4, 200: 4, 300: 3, 600: 2, 1100: 1}
# The far variant.  The stripe cell is the tile's largest reach (13 - 20 m with a giant in every scenario), and a tile leaves the
# stripe masks for the all-pairs fallback beyond 4000 cells: the scenarios at 2e5 and 7.5e5 m take the fallback, those at 3e4 m
# (1,500 - 2,300 cells) stay on the stripe masks, at large cell coordinates.  Nothing reports which one ran.
FAR_ORIGINS = (3.0e4, 2.0e5, -7.5e5)


def steps_of(E):
    return 40 if E <= 512 else 30


def giant_slot(bbox):
    """The slot of the scenario's largest box."""
    return int(np.argmax(0.5 * np.hypot(bbox[:, 0], bbox[:, 1])))


def _yard(E, r, steps, recipe, ego, origin):
    rng = np.random.default_rng([20250607, E, r, recipe == "mixed"])
    K = 6
    T = (steps + 2) * DT
    grid = np.linspace(0.0, T, K)
    side = np.sqrt((14.0 if recipe == "mixed" else 22.0) * E) + 4.0
    bbox = np.array([SMALL[i] for i in rng.choice(len(SMALL), E, p=SMALL_P)], np.float64)
    bbox[0] = EGO_BOXES[rng.integers(len(EGO_BOXES))]
    g = E - 1 if E > 64 else int(rng.integers(1, E))
    bbox[g] = GIANTS[0] if E > 64 else GIANTS[int(rng.integers(2))]
    etype = np.zeros(E, np.int32)
    kind = np.full(E, KIND_REPLAY, np.int32)
    kind[0] = KIND_AGENT_REPLAY if ego == "replay" or (ego == "sparse" and r % 4) else KIND_AGENT_PID
    is_ped = np.zeros(E, bool)
    if recipe == "mixed":  # pedestrian agents (social force) among vehicles of every class
        is_ped[1:] = rng.random(E - 1) < 0.4
        is_ped[g] = False
        is_ped[1 if g != 1 else 2] = True  # (at least one)
        kind[is_ped], etype[is_ped] = KIND_AGENT_PEDESTRIAN, 1
        veh = ~is_ped & (bbox == PED_BOX).all(axis=1)  # (the pedestrian-sized boxes of a mixed scene are its pedestrians)
        veh[0] = False
        bbox[veh] = np.array(SMALL)[rng.integers(1, len(SMALL), int(veh.sum()))]
        bbox[is_ped] = PED_BOX
    p0 = rng.uniform(-side / 2, side / 2, (E, 2))
    ang = rng.uniform(-np.pi, np.pi, E)
    speed = rng.uniform(0.0, 7.0, E)
    h0 = rng.uniform(-np.pi, np.pi, E)
    omega = np.where(rng.random(E) < 0.5, rng.uniform(-1.6, 1.6, E), rng.normal(0.0, 0.05, E))  # headings that turn
    p0[g] = rng.uniform(-side / 8, side / 8, 2)  # the giant crosses the middle of the yard
    speed[g] = rng.uniform(2.0, 5.0)
    p0[0] = rng.uniform(-side / 5, side / 5, 2)  # ... and the ego stays about it
    # escorts: small boxes that travel beside the giant's reference point
    esc = 1 + rng.choice(E - 1, min(8, E // 6), replace=False)
    esc = esc[esc != g]
    p0[esc], ang[esc] = p0[g] + rng.normal(0.0, 2.5, (len(esc), 2)), ang[g]
    speed[esc] = speed[g] * rng.uniform(0.8, 1.2, len(esc))
    u = rng.random(E)
    u[[0, g]] = 1.0  # the ego and the giant span the run
    static = u < 0.15
    partial = (~static) & (u < 0.4)  # entities that appear late, vanish early, or both
    ka = np.where(partial, rng.integers(0, K // 2, E), 0)
    kb = np.where(partial, rng.integers(K // 2, K, E), K - 1)
    ks = rng.integers(0, K, E)
    knots, off, routes, route_off = [], [0], [], [0]
    for e in range(E):
        idx = [ks[e]] if static[e] else list(range(ka[e], kb[e] + 1))
        if is_ped[e]:
            idx = [0, K - 1]
        rows = np.zeros((len(idx), 7))
        t = grid[idx]
        d = np.array([np.cos(ang[e]), np.sin(ang[e])])
        xy = p0[e] + speed[e] * (t[:, None] - T / 2) * d + rng.normal(0.0, 0.6, (len(idx), 2))
        if is_ped[e]:
            xy[:] = p0[e]
            goal = -p0[e] * rng.uniform(0.3, 1.0) + rng.normal(0.0, 2.0, 2)
            routes.append(np.stack([p0[e], goal]) + origin)
        route_off.append(route_off[-1] + (2 if is_ped[e] else 0))
        rows[:, 0], rows[:, 1:3], rows[:, 4] = t, xy + origin, h0[e] + omega[e] * t
        knots.append(rows)
        off.append(off[-1] + len(idx))
    sc = dict(knot_off=np.array(off, np.int64), knots=np.concatenate(knots), bbox=bbox, etype=etype, kind=kind, ego=0, t0=0.0,
              length=float(T), ctrl=None, giant=g)
    if recipe == "mixed":
        sc["route_off"] = np.array(route_off, np.int64)
        sc["routes"] = np.concatenate(routes) if routes else np.zeros((0, 2))
        sc["ped_ctrl"] = (is_ped, rng.uniform(0.5, 1.5, E) * 1.3, 3.0)
    return sc


_BATCHES = {}


def batch(recipe, E, ego="sparse", far=False):
    """The scenarios (plain arrays, as packing.pack_arrays takes them, + kind / giant) of one batch: recipe "yard" (replayed
    vehicles of every class) or "mixed" (four in ten of them pedestrian agents); ego "sparse" (a PID ego in every fourth
    scenario, the others replay), "pid" or "replay"; far: scenario r translated to (o, -o), o = FAR_ORIGINS[r % 3]."""
    key = (recipe, E, ego, far)
    if key not in _BATCHES:
        R = BATCH[E] if not far else 6
        _BATCHES[key] = [_yard(E, r, steps_of(E), recipe, ego, np.array([1.0, -1.0]) * (FAR_ORIGINS[r % 3] if far else 0.0))
                         for r in range(R)]
    return _BATCHES[key]


def ctrl_rows(sc, default_ctrl):
    """[E][NCTRL] controller rows of a scenario: the defaults, and the pedestrian agents' desired speed and radius."""
    ctrl = np.tile(np.asarray(default_ctrl, np.float64), (len(sc["kind"]), 1))
    if "ped_ctrl" in sc:
        is_ped, vdes, rad = sc["ped_ctrl"]
        ctrl[is_ped, C_PED_SPEED_DESIRED] = vdes[is_ped]
        ctrl[is_ped, C_PED_RADIUS] = rad
    return ctrl


# ---------------------------------------------------------------------------------------------------- the exact predicate
def _ints(A, B):
    """The 16 coordinates as integers over one common (power of two) denominator: exact."""
    fr = [Fraction(float(v)) for v in np.concatenate([np.asarray(A, np.float64).ravel(), np.asarray(B, np.float64).ravel()])]
    den = max(f.denominator for f in fr)
    v = [f.numerator * (den // f.denominator) for f in fr]
    return [(v[2 * i], v[2 * i + 1]) for i in range(4)], [(v[8 + 2 * i], v[9 + 2 * i]) for i in range(4)]


def _area2(q):
    return sum(q[i][0] * q[(i + 1) & 3][1] - q[(i + 1) & 3][0] * q[i][1] for i in range(4))


def quads_meet_exact(A, B):
    """Do the closed convex quads A, B ([4][2] fp64 corners in ring order) share a point?  Separating axes in exact rational
    arithmetic (the fp64 coordinates as fractions.Fraction, brought to one denominator): they are apart iff the projections
    on some edge normal are strictly apart; touching meets.  A quad without area (a segment) brings its edge directions as
    axes too -- the normals alone do not separate two collinear segments."""
    a, b = _ints(A, B)
    flat = _area2(a) == 0 or _area2(b) == 0
    for q in (a, b):
        for i in range(4):
            ex, ey = q[(i + 1) & 3][0] - q[i][0], q[(i + 1) & 3][1] - q[i][1]
            if ex == 0 and ey == 0:
                continue
            for nx, ny in ((-ey, ex), (ex, ey)) if flat else ((-ey, ex),):
                pa = [nx * x + ny * y for x, y in a]
                pb = [nx * x + ny * y for x, y in b]
                if max(pa) < min(pb) or max(pb) < min(pa):
                    return False
    return True


def near_pairs(cor, present):
    """(i, j), i < j, of the present entities whose bounding circles (centre = mean of the fp64 corners, radius = the
    farthest corner, both widened by far more than their rounding) touch: every other pair is apart, by construction."""
    idx = np.nonzero(present)[0]
    if len(idx) < 2:
        return np.zeros((0, 2), np.int64)
    c = cor[idx].mean(axis=1)
    scale = np.abs(cor[idx]).max() + 1.0
    rad = np.sqrt(((cor[idx] - c[:, None, :]) ** 2).sum(-1)).max(axis=1) * (1 + 1e-9) + 1e-9 * scale
    dx, dy = c[:, None, 0] - c[None, :, 0], c[:, None, 1] - c[None, :, 1]
    reach = (rad[:, None] + rad[None, :]) * (1 + 1e-9)
    ii, jj = np.nonzero(np.triu(dx * dx + dy * dy <= reach * reach, 1))
    return np.stack([idx[ii], idx[jj]], 1)


def corners_numpy(pose, bbox):
    """Entity.get_bounding_box_points with numpy's sin / cos, for whole tables at once ([...][6] poses, [...][4] boxes ->
    [...][4][2]; corners RR, FR, FL, RL).  For the TALLIES of modified box tables only, where an ulp of a sine decides
    nothing; every comparison goes through the oracle's corners."""
    pose, bbox = np.asarray(pose, np.float64), np.asarray(bbox, np.float64)
    W, L, cx, cy = (bbox[..., q, None] for q in range(4))
    s, c = np.sin(pose[..., 3, None]), np.cos(pose[..., 3, None])
    px = cx + 0.5 * L * np.array([-1.0, 1.0, 1.0, -1.0])
    py = cy + 0.5 * W * np.array([1.0, 1.0, -1.0, -1.0])
    return np.stack([pose[..., 0, None] + (px * c - py * s), pose[..., 1, None] + (px * s + py * c)], -1)


def corners_table(corners, poses, bbox):
    """[S][E][4][2] corners of recorded poses [S][E][6] (NaN = absent -> NaN corners) by `corners` (oracle.corners)."""
    S, E = poses.shape[:2]
    out = np.full((S, E, 4, 2), np.nan)
    for k in range(S):
        for e in np.nonzero(~np.isnan(poses[k, :, 0]))[0]:
            out[k, e] = corners(poses[k, e], bbox[e])
    return out


def _decided_in_fp64(A, B):
    """(apart, meet): bool [n] each, pairs [n][4][2] x 2 that fp64 decides beyond doubt.  Per edge normal n the gap between
    the two projections is computed in fp64; its rounding error is below 1e-14 * |n|_1 * (largest coordinate), and a gap
    counts as decided only beyond 1e-9 * that product.  Whatever is left goes to quads_meet_exact."""
    n_pairs = len(A)
    apart, doubt = np.zeros(n_pairs, bool), np.zeros(n_pairs, bool)
    scale = np.maximum(np.abs(A).max(axis=(1, 2)), np.abs(B).max(axis=(1, 2))) + 1.0
    for Q in (A, B):
        for i in range(4):
            e = Q[:, (i + 1) & 3] - Q[:, i]
            nx, ny = -e[:, 1], e[:, 0]
            pa = A[:, :, 0] * nx[:, None] + A[:, :, 1] * ny[:, None]
            pb = B[:, :, 0] * nx[:, None] + B[:, :, 1] * ny[:, None]
            gap = np.maximum(pb.min(1) - pa.max(1), pa.min(1) - pb.max(1))
            tol = 1e-9 * (np.abs(nx) + np.abs(ny)) * scale
            apart |= gap > tol
            doubt |= np.abs(gap) <= tol
    return apart, ~apart & ~doubt


_EXACT = {}
N_RATIONAL = [0]  # pairs that went to the rational arithmetic (a tally for the tests' printout)


def exact_pairs(key, cor):
    """{(step, i, j): bool} of every near pair of a corners table [S][E][4][2]: do the two boxes meet, exactly -- an fp64
    filter with a conservative margin (_decided_in_fp64), quads_meet_exact for every pair inside it; cached under `key`."""
    if key not in _EXACT:
        trip = [np.concatenate([np.full((len(p), 1), k), p], 1) for k in range(cor.shape[0])
                for p in [near_pairs(cor[k], ~np.isnan(cor[k, :, 0, 0]))] if len(p)]
        res = {}
        if trip:
            trip = np.concatenate(trip)
            A, B = cor[trip[:, 0], trip[:, 1]], cor[trip[:, 0], trip[:, 2]]
            apart, meet = _decided_in_fp64(A, B)
            for q in np.nonzero(~apart & ~meet)[0]:
                meet[q] = quads_meet_exact(A[q], B[q])
                N_RATIONAL[0] += 1
            res = {(int(k), int(i), int(j)): bool(m) for (k, i, j), m in zip(trip, meet)}
        _EXACT[key] = res
    return _EXACT[key]


MODS = ("center_y zeroed", "centre zeroed", "width and length swapped", "giant shrunk to the median box")


def modified_boxes(bbox, mod):
    """(the box table under one of MODS, the slots whose box changed)."""
    b = np.array(bbox, np.float64)
    if mod == MODS[0]:
        b[:, 3] = 0.0
    elif mod == MODS[1]:
        b[:, 2:] = 0.0
    elif mod == MODS[2]:
        b[:, [0, 1]] = b[:, [1, 0]]
    elif mod == MODS[3]:
        order = np.argsort(0.5 * np.hypot(b[:, 0], b[:, 1]), kind="stable")
        b[giant_slot(b)] = b[order[(len(b) - 1) // 2]]
    else:
        raise ValueError(mod)
    return b, np.nonzero((b != np.asarray(bbox)).any(axis=1))[0]


def decisive_pairs(key, corners, poses, bbox, mod):
    """The pair-steps whose exact answer flips under a modified box table: (lost, invented), lists of (step, i, j) -- pairs
    that meet with the true boxes (corners by `corners`, the oracle's) and not with the modified ones (corners_numpy), and
    the other way round."""
    base = exact_pairs(key, corners_table(corners, poses, bbox))
    b, changed = modified_boxes(bbox, mod)
    other = exact_pairs(key + (mod,), corners_numpy(poses, b[None]))
    ch = set(int(c) for c in changed)
    lost = [p for p, hit in base.items() if hit and (p[1] in ch or p[2] in ch) and not other.get(p, False)]
    invented = [p for p, hit in other.items() if hit and not base.get(p, False)]
    return lost, invented


def oracle_rollout(O, sc, steps, event_cap=64, **kw):
    """The scenario through the oracle for `steps` steps, every step recorded."""
    return O.rollout(sc["knot_off"], sc["knots"], sc["bbox"], sc["etype"], sc["kind"], sc["ego"], sc["t0"], sc["length"], DT,
                     ctrl=ctrl_rows(sc, O.DEFAULT_CTRL), max_steps=steps, record=True, event_cap=event_cap,
                     route_off=sc.get("route_off"), routes=sc.get("routes"), **kw)
