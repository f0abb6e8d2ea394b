"""Scenes of tests/test_surface_scan.py: the stripe network of tests/test_entity_status.py restated, the yards of
tests/box_scenes.py laid over it, and stationary entities standing on the adversarial points of tests/road_shapes.py.  A plain
module, like box_scenes.py."""
import numpy as np

import box_scenes as B
import road_shapes as S

(LAYER_DRIVEABLE, LAYER_ROAD, LAYER_INTERSECTION, LAYER_LANE, LAYER_WALKABLE, LAYER_PAVEMENT, LAYER_CROSSING,
 LAYER_IMPENETRABLE) = (1 << i for i in range(8))


def stripes():
    """Stripes over [-64, 64]^2 in periods of 8 m along x: a 4 m driveable rectangle (road), then a 4 m pavement."""
    rects, layers = [], []
    for k in range(16):
        x0 = -64.0 + 8.0 * k
        rects.append([(x0, -64.0), (x0 + 4.0, -64.0), (x0 + 4.0, 64.0), (x0, 64.0)])
        layers.append(LAYER_DRIVEABLE | LAYER_ROAD)
        rects.append([(x0 + 4.0, -64.0), (x0 + 8.0, -64.0), (x0 + 8.0, 64.0), (x0 + 4.0, 64.0)])
        layers.append(LAYER_WALKABLE | LAYER_PAVEMENT)
    n = len(rects)
    return dict(ring_off=np.arange(n + 1, dtype=np.int64), vert_off=4 * np.arange(n + 1, dtype=np.int64),
                verts=np.array(rects, np.float64).reshape(-1, 2), layers=np.array(layers, np.uint32))


def scene_network():
    """The network under the device scenes: the stripes, and over them what gives the other layers of the tests' lists a surface
    of their own -- a 2 m lane in the middle of every driveable stripe, and across the stripes, in periods of 8 m along y, a 4 m
    intersection band and a 2 m building.  The driveable, road, walkable and pavement surfaces are those of the stripes."""
    net = stripes()
    rects, layers = [], []
    for k in range(16):
        x0 = y0 = -64.0 + 8.0 * k
        rects.append([(x0 + 1.0, -64.0), (x0 + 3.0, -64.0), (x0 + 3.0, 64.0), (x0 + 1.0, 64.0)])
        layers.append(LAYER_LANE)
        rects.append([(-64.0, y0), (64.0, y0), (64.0, y0 + 4.0), (-64.0, y0 + 4.0)])
        layers.append(LAYER_INTERSECTION)
        rects.append([(-64.0, y0 + 5.0), (64.0, y0 + 5.0), (64.0, y0 + 7.0), (-64.0, y0 + 7.0)])
        layers.append(LAYER_IMPENETRABLE)
    n = len(net["layers"]) + len(rects)
    return dict(ring_off=np.arange(n + 1, dtype=np.int64), vert_off=4 * np.arange(n + 1, dtype=np.int64),
                verts=np.concatenate([net["verts"], np.array(rects, np.float64).reshape(-1, 2)]),
                layers=np.concatenate([net["layers"], np.array(layers, np.uint32)]))


def net_of(r):
    """One scenario in four has no network."""
    return -1 if r % 4 == 3 else 0


# ---------------------------------------------------------------------------------------------------- the yards
# (recipe, width, far): a nearly empty block, one slot in the second block, beyond the 512-slot tiles; and the far yards, which
# lie beside the stripes altogether
SCENES = (("yard", 3, False), ("yard", 65, False), ("yard", 520, False), ("yard", 65, True))
_SCENES = {}


def scenarios_of(recipe, E, far):
    """The scenarios of one device scene, at least four of them (net_of leaves the fourth without a network): box_scenes.batch
    where it has the width, else the same recipe."""
    key = (recipe, E, far)
    if key not in _SCENES:
        if far or E in B.BATCH:
            scs = B.batch(recipe, E, "sparse", far)
        else:
            scs = [B._yard(E, r, B.steps_of(E), recipe, "sparse", np.zeros(2)) for r in range(4)]
        _SCENES[key] = scs[:8 if E <= 3 else 4]
    return _SCENES[key]


def steps_of(E):
    """Six tenths of the run: the late entities have appeared and the early leavers have gone."""
    return (6 * B.steps_of(E)) // 10 + 2


def observers_of(R, E):
    """Every slot of every scenario, then a duplicated one, then the ego of every scenario (slot 0 in the yards)."""
    scen = np.concatenate([np.repeat(np.arange(R), E), [R - 1, R - 1], np.arange(R)]).astype(np.int32)
    slot = np.concatenate([np.tile(np.arange(E), R), [E - 1, E - 1], np.zeros(R)]).astype(np.int32)
    return scen, slot


# ---------------------------------------------------------------------------------------------------- adversarial networks
FAMILIES = ("holes", "thin", "degenerate", "traps")
PLACEMENTS = (0, 2, 4)  # road_shapes.PLACEMENTS: (0, 0), (4.5e5, 5.4e6), (2**40, -2**40)
ORIGIN_CLASSES = ("vertex", "midpoint", "on_axis_edge", "prolongation")  # on vertices, on edges, on prolongations of edges
PER_CLASS = 8
ADV_E = PER_CLASS * len(ORIGIN_CLASSES)
_ADV = {}


def adversarial_cases():
    """[(family, placement index, network arrays, origins [ADV_E][2], headings [ADV_E])], one per network that has vertices to
    stand on (the empty network of `degenerate` has none): PER_CLASS seeded points of each class of ORIGIN_CLASSES (repeated
    where a network has fewer), every other one turned to heading 0 -- beam 0 of a fan with angle0 = 0 then runs exactly along
    +x, through vertices and along axis-parallel edges -- and the rest turned two other ways."""
    if not _ADV:
        out = []
        for fam in FAMILIES:
            for pl in PLACEMENTS:
                assert S.PLACEMENTS[pl] in ((0.0, 0.0), (4.5e5, 5.4e6), (2.0 ** 40, -2.0 ** 40))
                nets = S.networks_of(fam, pl)
                for k, (arrays, (pts, cls)) in enumerate(zip(nets, S.points_of(fam, pl, nets))):
                    rng = np.random.default_rng([41, FAMILIES.index(fam), pl, k])
                    per_class = PER_CLASS if len(arrays["verts"]) <= 10000 else 2  # (the 60,000-vertex circle: the exact check is per edge)
                    picks = []
                    for name in ORIGIN_CLASSES:
                        q = pts[cls == S.CLASSES.index(name)]
                        q = q[np.isfinite(q).all(axis=1)]
                        if len(q):
                            picks.append(np.resize(q[rng.permutation(len(q))[:per_class]], (PER_CLASS, 2)))
                    if not picks:
                        continue
                    origins = np.resize(np.concatenate(picks), (ADV_E, 2))
                    head = np.where(np.arange(ADV_E) % 2 == 0, 0.0, 0.37 * (np.arange(ADV_E) % 4) - 3.0)
                    out.append((fam, pl, arrays, np.ascontiguousarray(origins), head))
        _ADV["cases"] = out
    return _ADV["cases"]


def standing(origins, headings):
    """bool [E]: the first entity of every distinct (origin, heading); the repeats of a network with few places to stand would
    only compute the same rows again (on the 60,000-vertex circle at some cost), so they enter the scene late and are absent."""
    _, first = np.unique(np.column_stack([origins, headings]), axis=0, return_index=True)
    out = np.zeros(len(origins), bool)
    out[first] = True
    return out


def standing_scenario(origins, headings):
    """Entities standing still at `origins` for 10 s (two identical knots each: the replayed pose is the knot, exactly); those
    that `standing` leaves out only from t = 5 s on."""
    E = len(origins)
    here = standing(origins, headings)
    knots, off = [], [0]
    for i in range(E):
        for t in (0.0 if here[i] else 5.0, 10.0):
            knots.append([t, origins[i, 0], origins[i, 1], 0.0, headings[i], 0.0, 0.0])
        off.append(len(knots))
    return dict(knot_off=np.array(off, np.int64), knots=np.array(knots), bbox=np.tile([2.0, 4.5, 0.0, 0.0], (E, 1)),
                etype=np.zeros(E, np.int32), ego=0, t0=0.0, length=10.0)
