"""Range-scan (lidar) observations (sg_range_scan, sg_range_scan_observers): a fan of beams from the pose point of the ego of
every scenario, or of any observer of sg_set_observers, each reporting the distance to the first other entity's box and the
rate at which it changes.  The reference has no such sensor, so the yardstick is `scan_reference` below -- a numpy restatement
of the definition in include/sgym.h (np.where for the selects, two products and a sum for every rotation, the oracle's
sin / cos) -- itself checked on hand-made scenes with exact answers and against an independent method (the beam against the
four edges of the box's corners).  Every device comparison is bit for bit on the features and exact on slots and hits."""
import os
import re

import numpy as np
import pytest

import box_scenes as B

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sg_range_scan", "sg_range_scan_observers")
SG_ERR_INVALID, SG_ERR_STATE = -1, -3
INF = float("inf")
PI = float(np.pi)

# The device scenes: yards of mixed boxes (tests/box_scenes.py), stepped until some entities have appeared and some have left.
# One fan serves every beam count: beam b of a shorter scan is beam b of the longest (a_b depends on angle0, dangle and b only),
# so the yardstick runs once per observer at 130 beams -- two turns of 65 -- and the shorter scans are its first beams.
WIDTHS = (3, 64, 65, 300, 520)  # an almost empty block, a full one, one entity in the second, five blocks, beyond the 512-slot tiles
N_RAYS = (1, 64, 65, 130)       # one beam, a full block of beams, one beam in the second, a partial third
ANGLE0, DANGLE = -PI, 2.0 * PI / 65.0
MAX_RANGE = 9.0  # a yard holds an entity per 14 - 22 m^2: at 9 m about a third of the beams end on nothing (the coverage guard below)
SCENES = [(recipe, E, False) for recipe in ("yard", "mixed") for E in WIDTHS] + [("yard", 65, True)]


@pytest.fixture
def sga():
    import scenario_gym_amd as sga

    return sga


# ---------------------------------------------------------------------------------------------------- the yardstick
def trig_of(oracle, angles):
    """(sin, cos) of every angle by the oracle's sincos: [..., 2]."""
    a = np.asarray(angles, np.float64)
    return np.array([oracle.sincos(x) for x in a.ravel()]).reshape(a.shape + (2,))


_BEAMS = {}


def beams_of(oracle, n_rays, angle0=ANGLE0, dangle=DANGLE):
    """(sin, cos) of a_b = angle0 + (double)b * dangle, b < n_rays: [n_rays, 2]."""
    key = (n_rays, angle0, dangle)
    if key not in _BEAMS:
        _BEAMS[key] = trig_of(oracle, np.float64(angle0) + np.arange(n_rays, dtype=np.float64) * np.float64(dangle))
    return _BEAMS[key]


def _slab(o, l, lo, hi):
    """The slab rule: o, lo, hi [E], l [B, E] -> (tn, tf) [B, E]."""
    t1, t2 = (lo - o) / l, (hi - o) / l
    inside = (o >= lo) & (o <= hi)
    up = t1 < t2
    return (np.where(l == 0.0, np.where(inside, -INF, INF), np.where(up, t1, t2)),
            np.where(l == 0.0, np.where(inside, INF, -INF), np.where(up, t2, t1)))


def scan_reference(poses, vels, present, bbox, trig, slot, beams, max_range):
    """The definition, for observer `slot` of one scenario: poses / vels [E, 6], present [E], bbox [E, 4] (width, length,
    center_x, center_y), trig [E, 2] (sin, cos of the headings), beams [B, 2] (sin, cos of the beam angles).  Returns (feat
    [B, 2], slots [B], hits).  numpy evaluates a * c + b * s as two products and a sum: no fused multiply-add."""
    n_rays, E = len(beams), len(present)
    feat, slots = np.zeros((n_rays, 2)), np.full(n_rays, -1, np.int32)
    if not present[slot]:
        return feat, slots, -1
    feat[:, 0] = max_range
    idx = np.nonzero(np.asarray(present, bool) & (np.arange(E) != slot))[0]  # every OTHER slot that is in State.poses
    if len(idx) == 0:
        return feat, slots, 0
    xo, yo, vxo, vyo = poses[slot, 0], poses[slot, 1], vels[slot, 0], vels[slot, 1]
    s, c = trig[slot]
    sb, cb = beams[:, 0, None], beams[:, 1, None]
    with np.errstate(all="ignore"):
        ux, uy = cb * c - sb * s, sb * c + cb * s  # [B, 1]
        se, ce = trig[idx, 0], trig[idx, 1]
        W, L, cx, cy = (bbox[idx, q] for q in range(4))
        dx, dy = xo - poses[idx, 0], yo - poses[idx, 1]
        ox, oy = dx * ce + dy * se, dy * ce - dx * se
        lx, ly = ux * ce + uy * se, uy * ce - ux * se  # [B, n]
        tnx, tfx = _slab(ox, lx, cx - 0.5 * L, cx + 0.5 * L)
        tny, tfy = _slab(oy, ly, cy - 0.5 * W, cy + 0.5 * W)
        tmin = np.zeros_like(lx)
        tmin = np.where(tnx > tmin, tnx, tmin)
        tmin = np.where(tny > tmin, tny, tmin)
        tmax = np.where(tfy < tfx, tfy, tfx)
        hit = (tmin <= tmax) & (tmin <= np.float64(max_range)) & (tmin < INF)
        rate = (vels[idx, 0] - vxo) * ux + (vels[idx, 1] - vyo) * uy
    first = np.argmin(np.where(hit, tmin, INF), axis=1)  # the smallest (tmin, slot): argmin takes the first of equals
    b = np.arange(n_rays)
    any_hit = hit[b, first]
    feat[any_hit, 0] = tmin[b, first][any_hit]
    feat[any_hit, 1] = rate[b, first][any_hit]
    slots[any_hit] = idx[first][any_hit]
    return feat, slots, int(any_hit.sum())


def reference_rows(st, bbox, trig, scen, slot, beams, max_range):
    """scan_reference for the observers (scen[i], slot[i]) of a batch state (RolloutEngine.state(raw=True))."""
    out = [scan_reference(st["poses"][r], st["vels"][r], st["present"][r], bbox[r], trig[r], e, beams, max_range) for r, e in zip(scen, slot)]
    n, nb = len(out), len(beams)
    return (np.array([o[0] for o in out]).reshape(n, nb, 2), np.array([o[1] for o in out], np.int32).reshape(n, nb),
            np.array([o[2] for o in out], np.int32))


def first_beams(want, m):
    """What the scan of the first m beams of the same fan gives."""
    feat, slots, hits = want
    return feat[:, :m], slots[:, :m], np.where(hits < 0, -1, (slots[:, :m] >= 0).sum(axis=1)).astype(np.int32)


def same(got, want):
    """feat bit for bit, slots and hits exactly."""
    return (got[0].shape == want[0].shape and np.ascontiguousarray(got[0]).tobytes() == np.ascontiguousarray(want[0]).tobytes()
            and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]))


# ---------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_the_range_scan_calls():
    """include/sgym.h declares both calls, _lib.SYMBOLS names them, and the ABI version is still 7 (a purely additive change)."""
    import scenario_gym_amd._lib as L

    header = open(os.path.join(ROOT, "include", "sgym.h")).read()
    assert L.ABI_VERSION == 7 and re.search(r"#define SG_ABI_VERSION 7\b", header)
    assert re.search(r"#define SG_SCAN_MAX_RAYS 1024\b", header)
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS
        assert re.search(r"\bint " + name + r"\(sg_handle \*h, int32_t n_rays, double angle0, double dangle, double max_range,\s*double \*feat,"
                         r"\s*int32_t \*slots,\s*int32_t \*hits, int32_t outputs_device\);", header), name


def _scene(xy, headings=None, vel=None, present=None, boxes=None):
    E = len(xy)
    poses, vels = np.zeros((E, 6)), np.zeros((E, 6))
    poses[:, :2] = xy
    if headings is not None:
        poses[:, 3] = headings
    if vel is not None:
        vels[:, :2] = vel
    bbox = np.tile([2.0, 4.0, 0.0, 0.0], (E, 1)) if boxes is None else np.asarray(boxes, np.float64)
    return poses, vels, np.ones(E, bool) if present is None else np.asarray(present, bool), bbox


def test_yardstick_on_hand_made_scenes(oracle):
    """The numpy restatement on scenes whose answers are worked out by hand.  Beam 0 points along the observer's heading
    (angle0 = 0: sin 0, cos 1 exactly), so lx = 1 and ly = 0 against a box of heading 0: the l == 0 slab."""
    ahead = beams_of(oracle, 1, 0.0, 0.0)
    assert ahead.tolist() == [[0.0, 1.0]]
    cross = beams_of(oracle, 4, 0.0, PI / 2)  # ahead, left, behind, right (up to the rounding of pi / 2)

    def scan(scene, slot=0, beams=ahead, max_range=100.0):
        poses, vels, present, bbox = scene
        return scan_reference(poses, vels, present, bbox, trig_of(oracle, poses[:, 3]), slot, beams, max_range)

    # a W = 2, L = 4 box centred at (10, 0): its rear face is 8 m ahead
    f, s, n = scan(_scene([(0, 0), (10, 0)]))
    assert f.tolist() == [[8.0, 0.0]] and s.tolist() == [1] and n == 1
    # ... the box off its reference point: center_x = 1.5 moves the rear face to 9.5, center_y = 3 moves the box off the beam
    assert scan(_scene([(0, 0), (10, 0)], boxes=[(2, 4, 0, 0), (2, 4, 1.5, 0.25)]))[0].tolist() == [[9.5, 0.0]]
    f, s, n = scan(_scene([(0, 0), (10, 0)], boxes=[(2, 4, 0, 0), (2, 4, 1.5, 3.0)]))
    assert f.tolist() == [[100.0, 0.0]] and s.tolist() == [-1] and n == 0 and not np.signbit(f[0, 1])
    # ... and the y-slab is inclusive: the beam runs along the box's flank at center_y = 1 (oy = 0 = lo)
    assert scan(_scene([(0, 0), (10, 0)], boxes=[(2, 4, 0, 0), (2, 4, 0, 1.0)]))[0].tolist() == [[8.0, 0.0]]
    assert scan(_scene([(0, 0), (10, 0)], boxes=[(2, 4, 0, 0), (2, 4, 0, np.nextafter(1.0, 2.0))]))[1].tolist() == [-1]
    # the origin inside a box, and on its boundary: 0.0 on every beam
    f, s, n = scan(_scene([(0, 0), (1, 0.5)]), beams=cross)
    assert f[:, 0].tolist() == [0.0] * 4 and s.tolist() == [1] * 4 and n == 4
    assert scan(_scene([(0, 0), (2, 0)]))[0].tolist() == [[0.0, 0.0]]
    # a box exactly at max_range is hit, one ulp beyond it is not
    assert scan(_scene([(0, 0), (10, 0)]), max_range=8.0)[1].tolist() == [1]
    f, s, n = scan(_scene([(0, 0), (10, 0)]), max_range=np.nextafter(8.0, 0.0))
    assert s.tolist() == [-1] and f[0, 0] == np.nextafter(8.0, 0.0) and n == 0
    assert scan(_scene([(0, 0), (np.nextafter(10.0, 11.0), 0)]), max_range=8.0)[1].tolist() == [-1]
    # two identical boxes in slots 3 and 5: slot 3; a nearer box occludes a farther one, whatever their slots
    far_away = (0, 50)
    f, s, n = scan(_scene([(0, 0), far_away, far_away, (10, 0), far_away, (10, 0)]))
    assert s.tolist() == [3] and f[0, 0] == 8.0
    assert scan(_scene([(0, 0), (20, 0), (10, 0)]))[1].tolist() == [2] and scan(_scene([(0, 0), (10, 0), (20, 0)]))[1].tolist() == [1]
    assert scan(_scene([(0, 0), (20, 0), (10, 0)]))[0].tolist() == [[8.0, 0.0]]
    # a zero-width box is a segment along its heading, a zero-length box one across it
    f, s, n = scan(_scene([(0, 0), (10, 0)], boxes=[(2, 4, 0, 0), (0, 4, 0, 0)]), beams=cross)
    assert s.tolist() == [1, -1, -1, -1] and f[0].tolist() == [8.0, 0.0]
    f, s, n = scan(_scene([(0, 0), (10, 0)], boxes=[(2, 4, 0, 0), (2, 0, 0, 0)]), beams=cross)
    assert s.tolist() == [1, -1, -1, -1] and f[0].tolist() == [10.0, 0.0]
    assert scan(_scene([(0, 0), (10, 2)], boxes=[(2, 4, 0, 0), (2, 0, 0, 0)]))[1].tolist() == [-1]
    # an absent target is not seen; an absent observer gets -1, -1 and +0.0
    assert scan(_scene([(0, 0), (10, 0), (20, 0)], present=[1, 0, 1]))[1].tolist() == [2]
    f, s, n = scan(_scene([(0, 0), (10, 0)], present=[0, 1]), beams=cross)
    assert n == -1 and s.tolist() == [-1] * 4 and not f.any() and not np.signbit(f).any()
    # the range rate: the target comes towards an observer that drives towards it -- negative, and the sum of both speeds
    f, s, n = scan(_scene([(0, 0), (10, 0)], vel=[(3, 0), (-2, 1)]))
    assert f.tolist() == [[8.0, -5.0]]
    f, s, n = scan(_scene([(0, 0), (10, 0)], vel=[(3, 0), (4.5, 0)]))
    assert f.tolist() == [[8.0, 1.5]]
    # the observer's heading turns the fan: heading pi / 2 looks along +y
    f, s, n = scan(_scene([(0, 0), (0, 10), (10, 0)], headings=[PI / 2, PI / 2, 0.0]), beams=cross)
    assert s.tolist() == [1, -1, -1, 2] and abs(f[0, 0] - 8.0) < 1e-14 and abs(f[3, 0] - 8.0) < 1e-14
    # max_range = +inf: a miss reports +inf, a hit however far its range
    f, s, n = scan(_scene([(0, 0), (1e9, 0)]), beams=cross, max_range=INF)
    assert s.tolist() == [1, -1, -1, -1] and f[:, 0].tolist() == [1e9 - 2.0, INF, INF, INF] and not f[:, 1].any()
    # a NaN anywhere in a target's pose: no hit
    assert scan(_scene([(0, 0), (np.nan, 0)]), max_range=INF)[1].tolist() == [-1]


def _ray_against_edges(o, u, quad, max_range):
    """The independent method: the beam o + t * u against the four edges of a box's corners [4][2]; 0 when o is inside."""
    d = np.roll(quad, -1, axis=0) - quad
    w = quad - o
    side = d[:, 0] * -w[:, 1] - d[:, 1] * -w[:, 0]  # cross(edge, o - corner)
    if (side >= 0).all() or (side <= 0).all():
        return 0.0
    den = u[0] * d[:, 1] - u[1] * d[:, 0]
    with np.errstate(all="ignore"):
        t = (w[:, 0] * d[:, 1] - w[:, 1] * d[:, 0]) / den
        q = (w[:, 0] * u[1] - w[:, 1] * u[0]) / den
    ok = (den != 0) & (t >= 0) & (q >= -1e-12) & (q <= 1 + 1e-12)
    return float(t[ok].min()) if ok.any() and t[ok].min() <= max_range else max_range


@pytest.mark.parametrize("E", [3, 6, 12, 24, 48, 100])
def test_yardstick_against_beam_edge_intersections(oracle, E):
    """On yard poses (every entity at the knot in the middle of its trajectory), 72 beams, max_range 25 m, for the ego and the
    giant of three scenarios: the slab test in the entity's frame and the beam against the four edges of
    box_scenes.corners_numpy give the same ranges within 1e-9."""
    n_rays, max_range = 72, 25.0
    beams = beams_of(oracle, n_rays, -PI, 2.0 * PI / n_rays)
    worst, hits, beams_seen = 0.0, 0, 0
    for sc in B.batch("yard", E)[:3]:
        off = sc["knot_off"]
        mid = (off[:-1] + off[1:] - 1) // 2
        poses, vels = sc["knots"][mid, 1:7], np.zeros((E, 6))
        present = np.ones(E, bool)
        trig = trig_of(oracle, poses[:, 3])
        quads = B.corners_numpy(poses, sc["bbox"])
        for slot in (0, sc["giant"]):
            feat, slots, n = scan_reference(poses, vels, present, sc["bbox"], trig, slot, beams, max_range)
            s, c = trig[slot]
            for b in range(n_rays):
                u = np.array([beams[b, 1] * c - beams[b, 0] * s, beams[b, 0] * c + beams[b, 1] * s])
                want = min(_ray_against_edges(poses[slot, :2], u, quads[e], max_range) for e in range(E) if e != slot)
                worst = max(worst, abs(feat[b, 0] - want))
            hits += n
            beams_seen += n_rays
    print(f"E={E}: {beams_seen} beams, {hits} hits, largest difference {worst:.3g}")
    assert worst <= 1e-9 and 0 < hits < beams_seen


# ---------------------------------------------------------------------------------------------------- the device scenes
_SCENES = {}


def scenarios_of(recipe, E, far):
    """The scenarios of one device scene: a few of box_scenes.batch (the widths it has no batch size for are built by the
    same recipe), as many as keep the yardstick's share of a test to a second or two."""
    key = (recipe, E, far)
    if key not in _SCENES:
        if far or E in B.BATCH:
            scs = B.batch(recipe, E, "sparse", far)
        else:
            scs = [B._yard(E, r, B.steps_of(E), recipe, "sparse", np.zeros(2)) for r in range(3)]
        _SCENES[key] = scs[:6 if E <= 3 or far else 3 if E <= 65 else 2 if E <= 300 else 1]
    return _SCENES[key]


def steps_of(E):
    """Six tenths of the run: the late entities have appeared and the early leavers have gone."""
    return (6 * B.steps_of(E)) // 10 + 2


def observers_of(scs, E):
    """Every entity of every scenario: the giant, boxes whose reference point lies outside them, entities that are not in the scene."""
    R = len(scs)
    return np.repeat(np.arange(R, dtype=np.int32), E), np.tile(np.arange(E, dtype=np.int32), R)


def test_device_scenes_exercise_the_kernel(oracle):
    """The coverage guard, by the yardstick alone on the oracle's states of the device scenes, every entity an observer: at
    least 20 % of the beams hit at a range > 0, at least 10 % miss, at least 1 % start inside a box."""
    beams = beams_of(oracle, max(N_RAYS))
    far_hits = misses = inside = total = absent = 0
    for recipe, E, far in SCENES:
        for sc in scenarios_of(recipe, E, far):
            k = steps_of(E)
            o = B.oracle_rollout(oracle, sc, k, force_steps=True)
            poses, vels = o["poses"][k], o["vels"][k]
            present = ~np.isnan(poses[:, 0])
            poses, vels = np.nan_to_num(poses), np.nan_to_num(vels)
            trig = trig_of(oracle, poses[:, 3])
            for slot in range(E):
                feat, slots, n = scan_reference(poses, vels, present, sc["bbox"], trig, slot, beams, MAX_RANGE)
                if n < 0:
                    absent += 1
                    continue
                total += len(beams)
                far_hits += int(((slots >= 0) & (feat[:, 0] > 0)).sum())
                inside += int(((slots >= 0) & (feat[:, 0] == 0)).sum())
                misses += int((slots < 0).sum())
    print(f"{total} beams: {far_hits / total:.1%} hit at a range > 0, {misses / total:.1%} miss, {inside / total:.1%} start inside a box; "
          f"{absent} observers not in the scene")
    assert far_hits >= 0.20 * total and misses >= 0.10 * total and inside >= 0.01 * total and absent > 0


# ---------------------------------------------------------------------------------------------------- GPU: the C ABI
GUARD = 64  # bytes of 0xCC kept on either side of every output buffer


def _cc(shape, dtype):
    """A host array whose every byte is 0xCC, with GUARD bytes of 0xCC on either side of it: (the array, its frame)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    frame = np.full(n + 2 * GUARD, 0xCC, np.uint8)
    return frame[GUARD:GUARD + n].view(dtype).reshape(shape), frame


def _guards_intact(*frames):
    return all((f[:GUARD] == 0xCC).all() and (f[-GUARD:] == 0xCC).all() for f in frames)


def _untouched(*frames):
    return all((f == 0xCC).all() for f in frames)


def _rewritten(*arrays):
    """No 0xCC word is left (no range, rate, slot or count of these scenes has that pattern)."""
    return all(not (a.view(np.uint32) == 0xCCCCCCCC).any() for a in arrays)


def _raw(eng, n, n_rays, max_range, observers, angle0=ANGLE0, dangle=DANGLE, want_slots=True, want_hits=True):
    """One of the two calls through ctypes into guarded 0xCC-filled host buffers of n observers: (rc, (feat, slots, hits), frames)."""
    (feat, f0), (slots, f1), (hits, f2) = _cc((n, n_rays, 2), np.float64), _cc((n, n_rays), np.int32), _cc((n,), np.int32)
    call = eng.lib.sg_range_scan_observers if observers else eng.lib.sg_range_scan
    rc = call(eng.h, n_rays, angle0, dangle, max_range, feat.ctypes.data, slots.ctypes.data if want_slots else None,
              hits.ctypes.data if want_hits else None, 0)
    return rc, (feat, slots, hits), (f0, f1, f2)


def _pack(scs):
    from scenario_gym_amd.engine import DEFAULT_CTRL
    from scenario_gym_amd.packing import pack_arrays

    return pack_arrays(scs, kinds=[s["kind"] for s in scs], ctrls=[B.ctrl_rows(s, DEFAULT_CTRL) for s in scs])


def _yard_engine(sga, scs, E, steps):
    """The scenarios on the device, `steps` steps on: (engine, raw state, bbox [R, E, 4])."""
    eng = sga.RolloutEngine(len(scs), E, timestep=B.DT, terminal_conditions=["max_length"], event_capacity=256)
    eng.upload(_pack(scs))
    eng.step(steps)
    return eng, eng.state(raw=True), np.array([s["bbox"] for s in scs])


@gpu
@pytest.mark.parametrize("recipe,E,far", SCENES, ids=[f"{r}-E{E}" + ("-far" if f else "") for r, E, f in SCENES])
def test_device_matches_the_yardstick(sga, oracle, recipe, E, far):
    """One device scene, stepped until entities have come and gone: the ego call and the observer call with every entity of
    every scenario an observer, at 1, 64, 65 and 130 beams, equal the yardstick; so does a scan without a range limit."""
    scs = scenarios_of(recipe, E, far)
    R = len(scs)
    eng, st, bbox = _yard_engine(sga, scs, E, steps_of(E))
    try:
        assert (not st["present"].all() or E <= 3) and st["present"][:, 0].all()
        trig = trig_of(oracle, st["poses"][..., 3])
        scen, slot = observers_of(scs, E)
        eng.set_observers(scen, slot)
        beams = beams_of(oracle, max(N_RAYS))
        want = reference_rows(st, bbox, trig, scen, slot, beams, MAX_RANGE)
        want_ego = tuple(a[slot == 0] for a in want)
        assert (want[2] > 0).any() and ((want[2] == -1).any() or E <= 3)
        for n_rays in N_RAYS:
            rc, got, frames = _raw(eng, R, n_rays, MAX_RANGE, observers=False)
            assert rc == 0 and same(got, first_beams(want_ego, n_rays)) and _guards_intact(*frames), ("egos", n_rays)
            rc, got, frames = _raw(eng, len(scen), n_rays, MAX_RANGE, observers=True)
            assert rc == 0 and same(got, first_beams(want, n_rays)) and _guards_intact(*frames), ("observers", n_rays)
        # no range limit: every entity of the scenario is within reach of every beam
        pick = np.unique(np.concatenate([np.nonzero(slot == 0)[0], np.arange(0, len(scen), max(len(scen) // 24, 1))]))
        eng.set_observers(scen[pick], slot[pick])
        rc, got, frames = _raw(eng, len(pick), 65, INF, observers=True)
        unlimited = reference_rows(st, bbox, trig, scen[pick], slot[pick], beams[:65], INF)
        assert rc == 0 and same(got, unlimited) and np.isinf(unlimited[0][..., 0][(unlimited[1] < 0) & (unlimited[2] >= 0)[:, None]]).all()
    finally:
        eng.close()


def _lattice_batch(sga, E=140):
    """Two scenarios of E entities standing still on a 7 m lattice, each turned its own way, with twins -- the same pose, the
    same box, another slot: 5 and 6 (neighbours), 3 and 67 (64 slots apart: the same lane of the next block), 10 and E - 1 (two
    blocks apart); one entity spawns late.  The ego is in the middle of the list."""
    from scenario_gym_amd.packing import pack_arrays

    side = int(np.ceil(np.sqrt(E)))
    twins = {6: 5, 67: 3, E - 1: 10}
    scs = []
    for r in range(2):
        xy = 7.0 * np.array([(i % side, i // side) for i in range(E)], np.float64) - (0.0 if r == 0 else 30.0)
        head = 0.37 * np.arange(E) - 3.0
        bbox = np.tile([2.0, 4.5, 0.0, 0.0], (E, 1)) + (np.arange(E) % 7)[:, None] * [0.1, 0.2, 0.15, -0.1]
        for hi, lo in twins.items():
            xy[hi], head[hi], bbox[hi] = xy[lo], head[lo], bbox[lo]
        knots, off = [], [0]
        for i in range(E):
            for t in (5.0 if i == 7 + r else 0.0, 10.0):
                knots.append([t, xy[i, 0], xy[i, 1], 0.0, head[i], 0.0, 0.0])
            off.append(len(knots))
        scs.append(dict(knot_off=np.array(off, np.int64), knots=np.array(knots), bbox=bbox, etype=np.zeros(E, np.int32),
                        ego=E // 2 + r, t0=0.0, length=10.0))
    packed = pack_arrays(scs)
    eng = sga.RolloutEngine(2, E, timestep=0.1)
    eng.upload(packed)
    eng.step(3)
    return eng, eng.state(raw=True), packed.bbox.reshape(2, E, 4).copy(), np.array([s["ego"] for s in scs], np.int32), twins


@gpu
def test_ties_go_to_the_lower_slot(sga, oracle):
    """A lattice with twins in other slots and other blocks of 64: whatever beam meets a pair reports the lower slot, never the
    higher; an observer sees its own twin at range 0."""
    E = 140
    eng, st, bbox, ego, twins = _lattice_batch(sga, E)
    try:
        assert not st["present"][0, 7] and not st["present"][1, 8] and st["present"].sum() == 2 * E - 2
        for hi, lo in twins.items():
            assert np.array_equal(st["poses"][:, hi], st["poses"][:, lo]) and np.array_equal(bbox[:, hi], bbox[:, lo])
        trig = trig_of(oracle, st["poses"][..., 3])
        scen, slot = observers_of([0, 1], E)
        eng.set_observers(scen, slot)
        n_rays = 130
        beams = beams_of(oracle, n_rays)
        for max_range in (25.0, INF):
            rc, got, _ = _raw(eng, 2, n_rays, max_range, observers=False)
            assert rc == 0 and same(got, reference_rows(st, bbox, trig, [0, 1], ego, beams, max_range)), max_range
            rc, got, _ = _raw(eng, len(scen), n_rays, max_range, observers=True)
            want = reference_rows(st, bbox, trig, scen, slot, beams, max_range)
            assert rc == 0 and same(got, want), max_range
            for hi, lo in twins.items():
                others = (slot != hi) & (slot != lo)
                assert (got[1][others] == lo).sum() > 20 and not (got[1][others] == hi).any(), (hi, lo)
                assert (got[1][slot == lo] == hi).all() and (got[0][slot == lo][..., 0] == 0.0).all()  # inside its twin
                assert (got[1][slot == hi] == lo).all()
    finally:
        eng.close()


@gpu
def test_observer_lists_output_paths_and_buffers(sga, oracle):
    """Duplicates and any order in the list; observers that are not in the scene; the observer (r, ego of r) gives the bytes of
    sg_range_scan; device outputs equal host outputs and are queued behind a step; every byte of 0xCC-filled buffers is
    rewritten and the guard bytes around them are not; NULL slots / hits are accepted; with no observers nothing is written;
    the calls answer for the state after sg_reset and after a further step."""
    import torch

    recipe, E = "yard", 64
    scs = scenarios_of(recipe, E, False)
    R, n_rays = len(scs), 65
    eng, st, bbox = _yard_engine(sga, scs, E, steps_of(E))
    try:
        beams = beams_of(oracle, n_rays)
        trig = trig_of(oracle, st["poses"][..., 3])
        rc, _, frames = _raw(eng, 4, n_rays, MAX_RANGE, observers=True)
        assert rc == 0 and _untouched(*frames)  # no observers set yet
        assert eng.lib.sg_range_scan_observers(eng.h, n_rays, ANGLE0, DANGLE, MAX_RANGE, None, None, None, 0) == 0
        absent = np.argwhere(~st["present"])
        assert len(absent) > 3 and (absent[:, 1] != 0).all()
        scen = np.concatenate([np.arange(R), [2, 2, 1, 0, 2], absent[:3, 0], np.ones(E, np.int64)]).astype(np.int32)
        slot = np.concatenate([np.zeros(R), [9, 9, 63, 31, 9], absent[:3, 1], np.arange(E)[::-1]]).astype(np.int32)
        eng.set_observers(scen, slot)
        n = len(scen)
        assert n % 4 != 0
        rc, host, frames = _raw(eng, n, n_rays, MAX_RANGE, observers=True)
        want = reference_rows(st, bbox, trig, scen, slot, beams, MAX_RANGE)
        assert rc == 0 and same(host, want) and _guards_intact(*frames) and _rewritten(*host)
        assert (want[2][R + 5:R + 8] == -1).all() and (host[1][R + 5:R + 8] == -1).all() and not host[0][R + 5:R + 8].any()
        assert host[0][R].tobytes() == host[0][R + 1].tobytes() == host[0][R + 4].tobytes()  # the duplicates
        rc, ego, frames = _raw(eng, R, n_rays, MAX_RANGE, observers=False)
        assert rc == 0 and all(a[:R].tobytes() == b.tobytes() for a, b in zip(host, ego)) and _guards_intact(*frames)
        # NULL slots / hits: the features alone, the other buffers untouched
        rc, (f, s, c), frames = _raw(eng, n, n_rays, MAX_RANGE, observers=True, want_slots=False, want_hits=False)
        assert rc == 0 and f.tobytes() == host[0].tobytes() and _untouched(frames[1], frames[2]) and _guards_intact(frames[0])
        rc, (f, s, c), frames = _raw(eng, R, n_rays, MAX_RANGE, observers=False, want_slots=False)
        assert rc == 0 and f.tobytes() == ego[0].tobytes() and _untouched(frames[1]) and np.array_equal(c, ego[2])
        rc, (f, s, c), frames = _raw(eng, n, n_rays, MAX_RANGE, observers=True, want_hits=False)
        assert rc == 0 and f.tobytes() == host[0].tobytes() and np.array_equal(s, host[1]) and _untouched(frames[2])
        # device outputs through the engine
        args = dict(n_rays=n_rays, angle0=ANGLE0, dangle=DANGLE, max_range=MAX_RANGE)
        for dev, ref in ((eng.range_scan_observers(torch_out=True, **args), host), (eng.range_scan(torch_out=True, **args), ego)):
            assert all(t.is_cuda for t in dev) and (dev[0].dtype, dev[1].dtype, dev[2].dtype) == (torch.float64, torch.int32, torch.int32)
            assert same([t.cpu().numpy() for t in dev], ref)
        assert same(eng.range_scan_observers(**args), host) and same(eng.range_scan(**args), ego)
        # ... and raw, into guarded 0xCC-filled device buffers, queued right behind a step
        sizes = (n * n_rays * 16, n * n_rays * 4, n * 4)
        d = [torch.full((b + 2 * GUARD,), 0xCC, dtype=torch.uint8, device="cuda:0") for b in sizes]
        torch.cuda.synchronize()
        assert eng.lib.sg_step(eng.h, 3, None, 0) == 0
        assert eng.lib.sg_range_scan_observers(eng.h, n_rays, ANGLE0, DANGLE, MAX_RANGE, *[t.data_ptr() + GUARD for t in d], 1) == 0
        assert eng.lib.sg_synchronize(eng.h) == 0
        st2 = eng.state(raw=True)
        assert int(st2["n_steps"].max()) == steps_of(E) + 3
        want2 = reference_rows(st2, bbox, trig_of(oracle, st2["poses"][..., 3]), scen, slot, beams, MAX_RANGE)
        back = [t.cpu().numpy() for t in d]
        got2 = (back[0][GUARD:-GUARD].view(np.float64).reshape(n, n_rays, 2), back[1][GUARD:-GUARD].view(np.int32).reshape(n, n_rays),
                back[2][GUARD:-GUARD].view(np.int32))
        assert same(got2, want2) and not same(want2, want) and _guards_intact(*back) and _rewritten(*got2)
        # after sg_reset, and a step further
        eng.reset()
        for more in (0, 1):
            if more:
                eng.step(1)
            st3 = eng.state(raw=True)
            assert int(st3["n_steps"].max()) == more
            want3 = reference_rows(st3, bbox, trig_of(oracle, st3["poses"][..., 3]), scen, slot, beams, MAX_RANGE)
            rc, got3, frames = _raw(eng, n, n_rays, MAX_RANGE, observers=True)
            assert rc == 0 and same(got3, want3) and not same(want3, want2)
            rc, ego3, frames = _raw(eng, R, n_rays, MAX_RANGE, observers=False)
            assert rc == 0 and all(a[:R].tobytes() == b.tobytes() for a, b in zip(got3, ego3))
        eng.set_observers([], [])
        rc, _, frames = _raw(eng, n, n_rays, MAX_RANGE, observers=True)
        assert rc == 0 and _untouched(*frames)
        assert same(eng.range_scan_observers(**args), (np.zeros((0, n_rays, 2)), np.zeros((0, n_rays), np.int32), np.zeros(0, np.int32)))
    finally:
        eng.close()


@gpu
def test_refusals_are_loud_and_leave_the_handle_working(sga, oracle):
    """SG_ERR_INVALID for n_rays outside 1..1024, an angle0 or dangle that is NaN or infinite, a max_range that is NaN or
    negative and a NULL feat, SG_ERR_STATE before sg_upload, each with a message that names the call and nothing written; the
    handle answers correctly afterwards, also at the largest beam count."""
    scs = scenarios_of("yard", 3, False)
    R, E = len(scs), 3
    fresh = sga.RolloutEngine(R, E, timestep=B.DT)
    for observers, name in ((False, "sg_range_scan"), (True, "sg_range_scan_observers")):
        rc, _, frames = _raw(fresh, R, 8, MAX_RANGE, observers)
        assert rc == SG_ERR_STATE and _untouched(*frames)
        assert fresh.lib.sg_last_error(fresh.h).decode().startswith(name + ":")
    fresh.close()
    eng, st, bbox = _yard_engine(sga, scs, E, 5)
    try:
        eng.set_observers([0, 1, 2], [1, 2, 1])
        nan = float("nan")
        bad = [(0, ANGLE0, DANGLE, 10.0), (-1, ANGLE0, DANGLE, 10.0), (1025, ANGLE0, DANGLE, 10.0), (8, nan, DANGLE, 10.0),
               (8, INF, DANGLE, 10.0), (8, -INF, DANGLE, 10.0), (8, ANGLE0, nan, 10.0), (8, ANGLE0, INF, 10.0), (8, ANGLE0, -INF, 10.0),
               (8, ANGLE0, DANGLE, nan), (8, ANGLE0, DANGLE, -1.0), (8, ANGLE0, DANGLE, -INF)]
        for observers, name in ((False, "sg_range_scan"), (True, "sg_range_scan_observers")):
            call = getattr(eng.lib, name)
            for n_rays, angle0, dangle, max_range in bad:
                (feat, f0), (slots, f1), (hits, f2) = _cc((R, 1100, 2), np.float64), _cc((R, 1100), np.int32), _cc((R,), np.int32)
                rc = call(eng.h, n_rays, angle0, dangle, max_range, feat.ctypes.data, slots.ctypes.data, hits.ctypes.data, 0)
                assert rc == SG_ERR_INVALID, (name, n_rays, angle0, dangle, max_range)
                assert eng.lib.sg_last_error(eng.h).decode().startswith(name + ":") and _untouched(f0, f1, f2)
            assert call(eng.h, 8, ANGLE0, DANGLE, 10.0, None, None, None, 0) == SG_ERR_INVALID
            assert eng.lib.sg_last_error(eng.h).decode().startswith(name + ":")
        trig = trig_of(oracle, st["poses"][..., 3])
        beams = beams_of(oracle, 1024, -PI, 2.0 * PI / 1024)
        rc, got, frames = _raw(eng, R, 1024, 0.0, observers=False, angle0=-PI, dangle=2.0 * PI / 1024)
        assert rc == 0 and same(got, reference_rows(st, bbox, trig, np.arange(R), np.zeros(R, int), beams, 0.0)) and _guards_intact(*frames)
        rc, got, frames = _raw(eng, 3, 1024, 15.0, observers=True, angle0=-PI, dangle=2.0 * PI / 1024)
        want = reference_rows(st, bbox, trig, [0, 1, 2], [1, 2, 1], beams, 15.0)
        assert rc == 0 and same(got, want) and _guards_intact(*frames) and (want[2] > 0).any()
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------- GPU: the Python layers
def _scenarios(sga, R, E, n_steps, seed, ego_at):
    """Scenario objects of a seeded synthetic batch with a shared road network; the entity with ref "ego" stands at position
    ego_at of the entity list.  Returns (scenarios, bbox [R, E, 4] in entity order)."""
    import road_shapes as S
    from scenario_gym_amd import BoundingBox, CatalogEntry, Entity, Scenario, Trajectory, synthetic
    from scenario_gym_amd.packing import unpack_scenario
    from scenario_gym_amd.road_network import RoadNetwork

    packed = synthetic.make_batch(R, E, n_steps=n_steps, timestep=0.1, n_knots=16, extent=20.0, vanish_frac=0.3, seed=seed)
    rn = RoadNetwork(name="lattice")
    rn._arrays = S.lattice(np.random.default_rng(11), offset=(-20.0, -20.0))[0]
    rng = np.random.default_rng(seed)
    scs, boxes = [], np.zeros((R, E, 4))
    for r in range(R):
        s = unpack_scenario(packed, r)
        order = list(range(E))
        order[0], order[ego_at] = order[ego_at], order[0]
        ents = []
        for j, i in enumerate(order):
            boxes[r, j] = (rng.uniform(1.0, 3.0), rng.uniform(3.0, 6.0), rng.uniform(-1.0, 1.5), rng.uniform(-0.5, 0.5))
            a, b = s["knot_off"][i], s["knot_off"][i + 1]
            ents.append(Entity(CatalogEntry(None, "x", None, "Vehicle", BoundingBox(*boxes[r, j])), Trajectory(s["knots"][a:b]),
                               ref="ego" if i == 0 else f"entity_{i}"))
        sc = Scenario(ents)
        sc.road_network = rn
        scs.append(sc)
    return scs, boxes


@gpu
def test_sensor_alone_and_combined_on_ego_and_other_agents(sga, oracle):
    """RangeScanSensor in a ScenarioGym rollout: alone on the ego's agent (the defaults), inside a CombinedSensor on the agent of
    another entity, and stepped by the caller, with State.range_scan beside them; what each saw equals the yardstick on the
    state it saw."""
    (sc,), boxes = _scenarios(sga, 1, 12, 30, seed=5, ego_at=4)
    assert sc.ego is sc.entities[4]
    other_ref = next(e.ref for e in sc.entities if e.ref != "ego" and e.trajectory.min_t <= 0.0 and e.trajectory.max_t >= 2.9)
    index = {e.ref: j for j, e in enumerate(sc.entities)}
    gym = sga.ScenarioGym(timestep=0.1)
    log = []

    def yardstick(slot, n_rays, angle0, dangle, max_range):
        st = gym._b.engine.state(raw=True)
        trig = trig_of(oracle, st["poses"][..., 3])
        return scan_reference(st["poses"][0], st["vels"][0], st["present"][0], boxes[0], trig[0], slot,
                              beams_of(oracle, n_rays, angle0, dangle), max_range)

    class Watcher(sga.Agent):
        def __init__(self, entity, sensor):
            super().__init__(entity, sga.ReplayTrajectoryController(entity), sensor)

        def _step(self, obs):
            if self.entity.ref == "ego":
                want = yardstick(4, 64, -PI, 2.0 * PI / 64, 100.0)
            else:
                want = yardstick(index[self.entity.ref], 33, -0.5, 1.0 / 32, 30.0)
            log.append((self.entity, obs, want))
            return sga.TeleportAction(pose=self.entity.trajectory.position_at_t(obs.next_t))

    def create_agent(s, e):
        if e.ref == "ego":
            return Watcher(e, sga.RangeScanSensor(e))
        if e.ref == other_ref:
            return Watcher(e, sga.CombinedSensor(e, sga.RangeScanSensor(e, n_rays=33, angle0=-0.5, dangle=1.0 / 32, max_range=30.0),
                                                 sga.FutureCollisionDetector(e, horizon=2.0)))

    gym.set_scenario(sc, create_agent=create_agent)
    ents = gym.state.scenario.entities
    ego, other = ents[4], ents[index[other_ref]]
    assert gym.state.scenario.ego is ego and sga.RangeScanSensor(ego).output_shape == (64, 2)
    loose = sga.RangeScanSensor(ents[2], n_rays=7, max_range=INF)  # stepped by the caller: joins the observers when first met

    def agrees(ranges, rates, hit, want):
        return (ranges.tobytes() == want[0][:, 0].tobytes() and rates.tobytes() == want[0][:, 1].tobytes()
                and hit == [ents[j] if j >= 0 else None for j in want[1]])

    for _ in range(6):
        gym.step()
        obs = loose.step(gym.state)
        assert isinstance(obs, sga.RangeScanObservation) and obs.entity is ents[2]
        assert agrees(obs.ranges, obs.range_rates, obs.hit_entities, yardstick(2, 7, -PI, 2.0 * PI / 7, INF))
        assert agrees(*gym.state.range_scan(16, 0.25, 0.125, 40.0), yardstick(4, 16, 0.25, 0.125, 40.0))
        assert agrees(*gym.state.range_scan(16, 0.25, 0.125, 40.0, entity=ego), yardstick(4, 16, 0.25, 0.125, 40.0))
        assert agrees(*gym.state.range_scan(5, entity=other), yardstick(index[other_ref], 5, -PI, 2.0 * PI / 5, 100.0))
    gym.close()
    seen = {id(ego): 0, id(other): 0}
    for entity, obs, want in log:
        assert obs.ranges.shape == ((64,) if entity is ego else (33,)) and agrees(obs.ranges, obs.range_rates, obs.hit_entities, want)
        assert obs.entity is entity and obs.pose is not None and entity not in obs.hit_entities
        if entity is other:
            assert isinstance(obs.future_collision, bool)
        seen[id(entity)] += sum(e is not None for e in obs.hit_entities)
    assert len(log) >= 10 and all(v > 5 for v in seen.values())


@gpu
def test_vector_env_range_scan(sga, oracle):
    """VectorScenarioEnv.range_scan / observe_entities_ranges, numpy and torch forms, after steps in which the short episodes
    ended and were reset: the yardstick on the state the environment is in."""
    short, box_s = _scenarios(sga, 2, 10, 5, seed=8, ego_at=3)
    long_, box_l = _scenarios(sga, 3, 10, 40, seed=9, ego_at=0)
    scs, bbox = short + long_, np.concatenate([box_s, box_l])
    ego = np.array([3, 3, 0, 0, 0], np.int32)
    lists = [[0, 1], [], [5, 5, 9], [2], [0, 7]]
    for torch_obs in (False, True):
        env = sga.VectorScenarioEnv(scs, timestep=0.1, n=8, terminal_conditions=["max_length"], torch_obs=torch_obs)
        env.reset()
        assert env.observe_entities_ranges(16)[0].shape[0] == 0  # no observers yet
        env.set_observers(lists)
        fired = np.zeros(5, bool)
        for _ in range(7):
            obs, reward, done, info = env.step(np.zeros((5, 2)))
            fired |= done
        assert fired[:2].all() and not fired[2:].any()
        st = env.engine.state(raw=True)
        trig = trig_of(oracle, st["poses"][..., 3])
        got = env.range_scan()
        *seen, env_of, slot = env.observe_entities_ranges(20, -1.0, 0.1, 35.0)
        if torch_obs:
            assert all(t.is_cuda for t in got) and all(t.is_cuda for t in seen) and env_of.is_cuda and slot.is_cuda
            got, seen = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in seen]
            env_of, slot = env_of.cpu().numpy(), slot.cpu().numpy()
        assert list(env_of) == [i for i, s in enumerate(lists) for _ in s] and list(slot) == [k for s in lists for k in s]
        assert same(got, reference_rows(st, bbox, trig, np.arange(5), ego, beams_of(oracle, 64, -PI, 2.0 * PI / 64), 100.0))
        assert (got[2] > 0).any() and got[0].shape == (5, 64, 2)
        assert same(seen, reference_rows(st, bbox, trig, env_of, slot, beams_of(oracle, 20, -1.0, 0.1), 35.0))
        env.close()
