"""The time to collision (sg_time_to_collision, sg_time_to_collision_observers): when the box of the ego of every scenario, or of
any observer of sg_set_observers, first touches another box if everybody keeps their velocity and heading, until when, with what
relative velocity and on which face -- and VectorScenarioEnv(driver_ttc=H), State.time_to_collision and MinTimeToCollision on top
of it.  The reference has nothing of the kind, so the yardstick is `ttc_reference` below: the definition of include/sgym.h
restated per pair (the same operations in the same order on fp64 values, np.where for the selects, the oracle's sincos), pinned
on hand-computed rows and checked against an independent method -- the exact rational separating-axis predicate of
tests/box_scenes.py on the oracle's corners a microsecond before and after the predicted contact.  Every device comparison is bit
for bit on the features and exact on the info."""
import os
import re

import numpy as np
import pytest

import box_scenes as B
import driver_scenes as DS
from test_entity_status import GUARD, _cc, _driver_objects, _guards_intact, _pack, _untouched, adjacency

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sg_time_to_collision", "sg_time_to_collision_observers")
SG_ERR_INVALID, SG_ERR_STATE = -1, -3
INF = float("inf")
NFEAT, NINFO = 4, 3

# The device scenes: the yards of mixed boxes (tests/box_scenes.py) at box_scenes.BATCH's batch sizes -- a nearly empty block, one
# row word, two row words, the eight-wavefront family, beyond the 512-slot tiles -- after 0, 10 and the last of steps_of(E) steps,
# every slot an observer, at the horizons 0, 2.5 and +inf.
WIDTHS = (3, 48, 100, 300, 600)
RECIPES = ("yard", "mixed")
SCENES = [(recipe, E) for recipe in RECIPES for E in WIDTHS]
HORIZONS = (0.0, 2.5, INF)


def states_of(E):
    return (0, 10, B.steps_of(E))


@pytest.fixture
def sga():
    import scenario_gym_amd as sga

    return sga


# ---------------------------------------------------------------------------------------------------- the yardstick
def pair_slabs(xo, yo, s, c, vxo, vyo, Wo, Lo, cxo, cyo, xe, ye, sn, cn, vxe, vye, We, Le, cxe, cye):
    """The per-pair quantities and the four slabs of the definition, for fp64 scalars or arrays that broadcast: (tmin, tmax, axis,
    o [4], l [4], H [4], nan) before the contact rule and the collision bit.  Every line is one line of the header."""
    with np.errstate(all="ignore"):
        px, py = xo + (cxo * c - cyo * s), yo + (cxo * s + cyo * c)
        qx, qy = xe + (cxe * cn - cye * sn), ye + (cxe * sn + cye * cn)
        dx, dy, wx, wy = qx - px, qy - py, vxe - vxo, vye - vyo
        cr, sr = cn * c + sn * s, sn * c - cn * s
        o = [dx * c + dy * s, dy * c - dx * s, dx * cn + dy * sn, dy * cn - dx * sn]
        l = [wx * c + wy * s, wy * c - wx * s, wx * cn + wy * sn, wy * cn - wx * sn]
        H = [0.5 * Lo + 0.5 * (np.abs(Le * cr) + np.abs(We * sr)), 0.5 * Wo + 0.5 * (np.abs(Le * sr) + np.abs(We * cr)),
             0.5 * Le + 0.5 * (np.abs(Lo * cr) + np.abs(Wo * sr)), 0.5 * We + 0.5 * (np.abs(Lo * sr) + np.abs(Wo * cr))]
        shape = np.broadcast(o[0], l[0], H[0]).shape
        tmin, tmax, axis, nan = np.zeros(shape), np.full(shape, INF), np.full(shape, -1), np.zeros(shape, bool)
        for i in range(4):
            t1, t2 = (-H[i] - o[i]) / l[i], (H[i] - o[i]) / l[i]
            still, inside, up = l[i] == 0.0, np.abs(o[i]) <= H[i], t1 < t2
            tn = np.where(still, np.where(inside, -INF, INF), np.where(up, t1, t2))
            tf = np.where(still, np.where(inside, INF, -INF), np.where(up, t2, t1))
            nan = nan | np.isnan(o[i]) | np.isnan(l[i]) | np.isnan(H[i])
            take = tn > tmin  # the first strictly larger value wins
            tmin, axis = np.where(take, tn, tmin), np.where(take, i, axis)
            tmax = np.where(tf < tmax, tf, tmax)
    return tmin, tmax, axis, o, l, H, nan


class TtcScene:
    """The slabs of every (observer, other) pair of ONE scenario's state, computed once for all its observers and horizons: poses /
    vels [E, 6], present [E], coll [E] or [E, words], bbox [E, 4]."""

    def __init__(self, oracle, poses, vels, present, coll, bbox):
        E = len(present)
        poses, vels, bbox = np.asarray(poses, np.float64), np.asarray(vels, np.float64), np.asarray(bbox, np.float64)
        self.E, self.present = E, np.asarray(present, bool)
        self.bit = adjacency(coll, E)[:, :E] != 0
        sc = np.array([oracle.sincos(h) for h in poses[:, 3]]).reshape(E, 2)
        cols = (poses[:, 0], poses[:, 1], sc[:, 0], sc[:, 1], vels[:, 0], vels[:, 1], bbox[:, 0], bbox[:, 1], bbox[:, 2], bbox[:, 3])
        self.tmin, self.tmax, self.axis, _, l, _, self.nan = pair_slabs(*[q[:, None] for q in cols], *[q[None, :] for q in cols])
        self.l0, self.l1 = l[0], l[1]

    def row(self, o, horizon):
        """(feat [4], info [3]) of observer slot o."""
        if not self.present[o]:
            return [0.0, 0.0, 0.0, 0.0], [-1, -1, -1]
        cand = self.present & (np.arange(self.E) != o)  # every OTHER slot that is in State.poses
        bit = self.bit[o]
        meets = ~self.nan[o] & (self.tmin[o] <= self.tmax[o]) & (self.tmin[o] <= horizon) & (self.tmin[o] < INF)
        contact = cand & (bit | meets)
        if not contact.any():
            return [INF, 0.0, 0.0, 0.0], [-1, 0, -1]
        tmin = np.where(bit, 0.0, self.tmin[o])  # the state's own predicate decides the present
        e = int(np.argmin(np.where(contact, tmin, INF)))  # the smallest (tmin, slot): argmin takes the first of equals
        t, until = float(tmin[e]), float(self.tmax[o, e])
        return [t, until if until > t else t, float(self.l0[o, e]), float(self.l1[o, e])], [e, int(contact.sum()), -1 if bit[e] else int(self.axis[o, e])]


def ttc_scenes(oracle, st, bbox, scenarios):
    """{r: TtcScene} of the scenarios `scenarios` of a batch state as RolloutEngine.state(raw=True) gives it; bbox [R, E, 4]."""
    return {int(r): TtcScene(oracle, st["poses"][r], st["vels"][r], st["present"][r], st["coll"][r], bbox[r]) for r in np.unique(scenarios)}


def ttc_reference(oracle, st, bbox, scen, slot, horizon, scenes=None):
    """The definition for the observers (scen[i], slot[i]) of a batch state: (feat [n, 4], info [n, 3] int32).  scenes: the
    ttc_scenes of this state, when several horizons are asked of it."""
    scen, slot = np.asarray(scen, np.int64), np.asarray(slot, np.int64)
    scenes = ttc_scenes(oracle, st, bbox, scen) if scenes is None else scenes
    feat, info = np.zeros((len(scen), NFEAT)), np.zeros((len(scen), NINFO), np.int32)
    done = {}
    for i, (r, o) in enumerate(zip(scen.tolist(), slot.tolist())):
        if (r, o) not in done:
            done[(r, o)] = scenes[r].row(o, horizon)
        feat[i], info[i] = done[(r, o)]
    return feat, info


def same(got, want):
    """feat bit for bit, info exactly."""
    return (got[0].shape == want[0].shape and np.ascontiguousarray(got[0]).tobytes() == np.ascontiguousarray(want[0]).tobytes()
            and np.array_equal(got[1], want[1]))


# ---------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_the_ttc_calls():
    """include/sgym.h declares both calls and the SG_TTC_* widths, _lib.SYMBOLS names them, and the ABI version is still 7."""
    import scenario_gym_amd._lib as L

    header = open(os.path.join(ROOT, "include", "sgym.h")).read()
    assert L.ABI_VERSION == 7 and re.search(r"#define SG_ABI_VERSION 7\b", header)
    assert re.search(r"#define SG_TTC_NFEAT\s+4\b", header) and re.search(r"#define SG_TTC_NINFO\s+3\b", header)
    assert (L.TTC_NFEAT, L.TTC_NINFO) == (NFEAT, NINFO)
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS
        assert re.search(r"\bint " + name + r"\(sg_handle \*h, double horizon, double \*feat, int32_t \*info, int32_t outputs_device\);", header), name


def _scene(oracle, xy, boxes, vel, headings=None, present=None, coll=None):
    E = len(xy)
    poses, vels = np.zeros((E, 6)), np.zeros((E, 6))
    poses[:, :2], vels[:, :2] = xy, vel
    if headings is not None:
        poses[:, 3] = headings
    return TtcScene(oracle, poses, vels, np.ones(E, bool) if present is None else present, np.zeros(E, np.uint64) if coll is None else coll, boxes)


def test_yardstick_on_hand_computed_rows(oracle):
    """The restatement on pairs whose answers are worked out by hand (heading 0: sin 0, cos 1 exactly)."""
    car = (2.0, 4.0, 0.0, 0.0)  # width, length: half extents 1 and 2
    head_on = dict(xy=[(0, 0), (20, 0)], boxes=[car, car], vel=[(5, 0), (-5, 0)])
    # centres 20 m apart, closing at 10 m/s, H = 2 + 2 along: contact from (20 - 4) / 10 to (20 + 4) / 10; the tie with the other
    # box's own along axis keeps axis 0
    assert _scene(oracle, **head_on).row(0, 5.0) == ([1.6, 2.4, -10.0, 0.0], [1, 1, 0])
    assert _scene(oracle, **head_on).row(1, 5.0) == ([1.6, 2.4, 10.0, 0.0], [0, 1, 0])
    # ... the other one turned round (sin pi is 1.2e-16: the across axes move by 1e-15 and decide nothing)
    f, i = _scene(oracle, headings=[0.0, np.pi], **head_on).row(0, 5.0)
    assert f == [1.6, 2.4, -10.0, 0.0] and i == [1, 1, 0]
    # a 3 m lateral offset against H = 1 + 1 across: they pass
    assert _scene(oracle, [(0, 0), (20, 3)], [car, car], [(5, 0), (-5, 0)]).row(0, 5.0) == ([INF, 0.0, 0.0, 0.0], [-1, 0, -1])
    assert _scene(oracle, [(0, 0), (20, 2)], [car, car], [(5, 0), (-5, 0)]).row(0, 5.0)[0][:2] == [1.6, 2.4]  # (2 m: the sides touch, inclusive)
    # a crossing pair at 90 degrees, H = 2 + 1 on both of the observer's axes: along [1.7, 2.3], across [1.9, 2.5] -- its side is met
    cross = _scene(oracle, [(0, 0), (20, -22)], [car, car], [(10, 0), (0, 10)], headings=[0.0, np.pi / 2])
    assert cross.row(0, 5.0) == ([1.9, 2.3, -10.0, 10.0], [1, 1, 1])
    f, i = cross.row(1, 5.0)  # seen from the other: its front meets first (its along axis is the observer's across axis)
    assert f[:2] == [1.9, 2.3] and i == [0, 1, 0] and abs(f[2] + 10.0) < 1e-14 and abs(f[3] + 10.0) < 1e-14
    # a parallel pair at equal speed: l == 0 on every axis
    assert _scene(oracle, [(0, 0), (0, 5)], [car, car], [(7, 0), (7, 0)]).row(0, INF) == ([INF, 0.0, 0.0, 0.0], [-1, 0, -1])
    assert _scene(oracle, [(0, 0), (1, 1)], [car, car], [(7, 0), (7, 0)]).row(0, 0.0) == ([0.0, INF, 0.0, 0.0], [1, 1, -1])  # ... overlapping for ever
    # the collision bit: +0.0 and face -1 whatever the slabs say -- here they say 1.6
    f, i = _scene(oracle, coll=np.array([2, 1], np.uint64), **head_on).row(0, 5.0)
    assert f == [0.0, 2.4, -10.0, 0.0] and not np.signbit(f[0]) and i == [1, 1, -1]
    f, i = _scene(oracle, [(0, 0), (0, 50)], [car, car], [(0, 0), (np.nan, 0)], coll=np.array([2, 1], np.uint64)).row(0, 0.0)
    assert f[:2] == [0.0, INF] and i == [1, 1, -1]  # ... or cannot say
    # ... and a set bit beats an earlier slot that is 1.6 s away, an unset one loses to it
    three = dict(xy=[(0, 0), (20, 0), (0, 30)], boxes=[car] * 3, vel=[(5, 0), (-5, 0), (5, 0)])
    assert _scene(oracle, coll=np.array([4, 0, 1], np.uint64), **three).row(0, 5.0) == ([0.0, 0.0, 0.0, 0.0], [2, 2, -1])  # (tmax = -inf there: until = tmin)
    assert _scene(oracle, **three).row(0, 5.0)[1] == [1, 1, 0]
    # the horizon is inclusive: exactly tmin is a contact, one ulp below is none
    assert _scene(oracle, **head_on).row(0, 1.6)[1] == [1, 1, 0]
    assert _scene(oracle, **head_on).row(0, float(np.nextafter(1.6, 0.0))) == ([INF, 0.0, 0.0, 0.0], [-1, 0, -1])
    assert _scene(oracle, **head_on).row(0, INF)[0][0] == 1.6 and _scene(oracle, **head_on).row(0, 0.0)[1] == [-1, 0, -1]
    # horizon 0 keeps what overlaps now, with or without the bit
    assert _scene(oracle, [(0, 0), (3, 0)], [car, car], [(5, 0), (-5, 0)]).row(0, 0.0) == ([0.0, 0.7, -10.0, 0.0], [1, 1, -1])
    # a zero-width box is a segment along its heading, a zero-length box one across it
    thin, flat = (0.0, 4.0, 0.0, 0.0), (2.0, 0.0, 0.0, 0.0)
    assert _scene(oracle, [(0, 0), (20, 1)], [car, thin], [(5, 0), (-5, 0)]).row(0, 5.0) == ([1.6, 2.4, -10.0, 0.0], [1, 1, 0])  # (H = 1 + 0 across: touching)
    assert _scene(oracle, [(0, 0), (20, 1.5)], [car, thin], [(5, 0), (-5, 0)]).row(0, 5.0)[1] == [-1, 0, -1]
    assert _scene(oracle, [(0, 0), (20, 0)], [car, flat], [(5, 0), (-5, 0)]).row(0, 5.0) == ([1.8, 2.2, -10.0, 0.0], [1, 1, 0])  # (H = 2 + 0 along)
    assert _scene(oracle, [(0, 0), (20, 0)], [thin, flat], [(5, 0), (-5, 0)]).row(1, 5.0) == ([1.8, 2.2, 10.0, 0.0], [0, 1, 0])
    # a NaN velocity: no contact, and the entity behind it is found
    f, i = _scene(oracle, [(0, 0), (10, 0), (20, 0)], [car] * 3, [(5, 0), (np.nan, 0), (-5, 0)]).row(0, 5.0)
    assert f == [1.6, 2.4, -10.0, 0.0] and i == [2, 1, 0]
    # a tie in tmin between two slots goes to the lower slot; the count sees both; an absent slot is no candidate
    tie = dict(xy=[(0, 0), (50, 50), (20, -0.5), (20, 0.5)], boxes=[car] * 4, vel=[(5, 0), (5, 0), (-5, 0), (-5, 0)])
    assert _scene(oracle, **tie).row(0, 5.0) == ([1.6, 2.4, -10.0, 0.0], [2, 2, 0])
    assert _scene(oracle, present=np.array([1, 1, 0, 1], bool), **tie).row(0, 5.0)[1] == [3, 1, 0]
    # an absent observer; a lone one
    assert _scene(oracle, present=np.array([0, 1, 1, 1], bool), **tie).row(0, 5.0) == ([0.0] * 4, [-1, -1, -1])
    assert _scene(oracle, [(0, 0)], [car], [(5, 0)]).row(0, INF) == ([INF, 0.0, 0.0, 0.0], [-1, 0, -1])
    # an off-centre box: the centre, not the pose point, is what moves -- (1.37, 0) ahead of it on both, so 20 m apart still
    off = (2.0, 4.0, 1.37, 0.0)
    assert _scene(oracle, [(0, 0), (20, 0)], [off, off], [(5, 0), (-5, 0)]).row(0, 5.0)[0][:2] == [1.6, 2.4]
    assert _scene(oracle, [(0, 0), (20, 0)], [off, car], [(5, 0), (-5, 0)]).row(0, 5.0)[0][0] == (-4.0 + (20.0 - 1.37)) / 10.0


def _meet_exact(A, Bq):
    """Do the quads A[k] and Bq[k] ([n, 4, 2] fp64 corners) share a point, exactly: the fp64 filter of box_scenes with its
    conservative margin, the rational separating-axis predicate for every pair inside it (box_scenes.exact_pairs does the same)."""
    apart, meet = B._decided_in_fp64(A, Bq)
    for q in np.nonzero(~apart & ~meet)[0]:
        meet[q] = B.quads_meet_exact(A[q], Bq[q])
    return meet


def test_yardstick_against_the_exact_predicate(oracle):
    """40,000 seeded random pairs, horizon 5 s.  A contact with tmin > 0: both boxes' oracle corners translated to tmin - d and
    tmin + d, d = 1e-6 s -- the exact predicate says disjoint before and overlapping after; a contact at tmin == 0: overlapping now;
    no contact: disjoint at 11 evenly spaced times in [0, 5].  Left out are the contacts the two probes cannot separate: shorter
    than 4 d, sooner than 2 d, or closing so slowly on the deciding axis that d moves the boxes by less than 1e-9 m -- at most 1 %
    of the contacts."""
    n, horizon, d = 40000, 5.0, 1e-6
    rng = np.random.default_rng(7)
    pose = np.zeros((2, n, 6))
    pose[..., :2], pose[..., 3] = rng.uniform(-40.0, 40.0, (2, n, 2)), rng.uniform(-np.pi, np.pi, (2, n))
    vel = rng.uniform(-15.0, 15.0, (2, n, 2))
    box = np.stack([rng.uniform(0.4, 3.0, (2, n)), rng.uniform(0.4, 16.0, (2, n)), rng.uniform(-2.0, 2.0, (2, n)), rng.uniform(-1.0, 1.0, (2, n))], -1)
    sc = np.array([[oracle.sincos(h) for h in pose[k, :, 3]] for k in range(2)])
    cols = lambda k: (pose[k, :, 0], pose[k, :, 1], sc[k, :, 0], sc[k, :, 1], vel[k, :, 0], vel[k, :, 1], box[k, :, 0], box[k, :, 1], box[k, :, 2], box[k, :, 3])  # noqa: E731
    tmin, tmax, axis, _, l, _, nan = pair_slabs(*cols(0), *cols(1))
    contact = ~nan & (tmin <= tmax) & (tmin <= horizon) & (tmin < INF)
    cor = np.array([[oracle.corners(pose[k, q], box[k, q]) for q in range(n)] for k in range(2)])  # [2, n, 4, 2] at t = 0
    at = lambda k, idx, t: cor[k, idx] + (vel[k, idx] * np.asarray(t)[..., None])[:, None, :]  # noqa: E731
    later = np.nonzero(contact & (tmin > 0.0))[0]
    l_dec = np.abs(np.choose(np.maximum(axis[later], 0), [q[later] for q in l]))
    left_out = (tmax[later] - tmin[later] < 4 * d) | (tmin[later] < 2 * d) | (l_dec * d < 1e-9)
    probe = later[~left_out]
    before = _meet_exact(at(0, probe, tmin[probe] - d), at(1, probe, tmin[probe] - d))
    after = _meet_exact(at(0, probe, tmin[probe] + d), at(1, probe, tmin[probe] + d))
    now = np.nonzero(contact & (tmin == 0.0))[0]
    overlapping = _meet_exact(cor[0, now], cor[1, now])
    print(f"{int(contact.sum())} contacts of {n} pairs, {len(now)} of them already overlapping, {int(left_out.sum())} left out, "
          f"{int(before.sum())} meet before, {int((~after).sum())} apart after, {int((~overlapping).sum())} apart now; faces {np.bincount(axis[later] + 1, minlength=5).tolist()}")
    assert contact.sum() >= 2000 and len(now) >= 300 and (np.bincount(axis[later], minlength=4) >= 100).all()
    assert left_out.sum() <= 0.01 * contact.sum()
    assert not before.any() and after.all() and overlapping.all()
    none = np.nonzero(~contact)[0]
    for t in np.linspace(0.0, horizon, 11):
        met = _meet_exact(at(0, none, np.full(len(none), t)), at(1, none, np.full(len(none), t)))
        assert not met.any(), (t, none[met][:4])


# ---------------------------------------------------------------------------------------------------- GPU: the C ABI
def _raw(eng, n, observers, horizon, want_info=True, want_feat=True, device=0):
    """One of the two calls through ctypes into guarded 0xCC-filled host buffers of n observers: (rc, (feat, info), frames)."""
    (feat, f0), (info, f1) = _cc((n, NFEAT), np.float64), _cc((n, NINFO), np.int32)
    call = eng.lib.sg_time_to_collision_observers if observers else eng.lib.sg_time_to_collision
    rc = call(eng.h, horizon, feat.ctypes.data if want_feat else None, info.ctypes.data if want_info else None, device)
    return rc, (feat, info), (f0, f1)


def _yard_engine(sga, scs, E):
    eng = sga.RolloutEngine(len(scs), E, timestep=B.DT, terminal_conditions=["max_length"], event_capacity=256)
    eng.upload(_pack(scs))
    eng.reset()
    return eng, np.array([s["bbox"] for s in scs])


def _observers(R, E):
    """Every slot of every scenario, then a duplicated one, then the ego of every scenario (slot 0 in the yards)."""
    scen = np.concatenate([np.repeat(np.arange(R), E), [R - 1, R - 1], np.arange(R)]).astype(np.int32)
    slot = np.concatenate([np.tile(np.arange(E), R), [E - 1, E - 1], np.zeros(R)]).astype(np.int32)
    return scen, slot


def _mismatches(got, want, scen, slot):
    bad = np.nonzero((got[0].view(np.uint64) != want[0].view(np.uint64)).any(1) | (got[1] != want[1]).any(1))[0]
    return [(int(scen[i]), int(slot[i]), got[0][i].tolist(), want[0][i].tolist(), got[1][i].tolist(), want[1][i].tolist()) for i in bad[:4]]


@gpu
@pytest.mark.parametrize("recipe,E", SCENES, ids=[f"{r}-E{E}" for r, E in SCENES])
def test_device_matches_the_yardstick(sga, oracle, recipe, E):
    """One device scene after 0, 10 and the last of its steps, at the horizons 0, 2.5 and +inf: the ego call and the observer call
    with every slot of every scenario an observer (a duplicate and the egos behind them), host and device outputs -- all equal the
    yardstick on the state the device holds, the ego rows of the observer call are the bytes of the ego call, and the duplicates
    get the same rows.  The guards against a vacuous pass: over the scene some observers are absent (but for the mixed yard of 3
    slots, where nobody can be), some have no threat within 2.5 s, some overlap now, every face meets first somewhere, and some
    observer meets two or more."""
    scs = B.batch(recipe, E)
    R = len(scs)
    eng, bbox = _yard_engine(sga, scs, E)
    try:
        scen, slot = _observers(R, E)
        n = len(scen)
        eng.set_observers(scen, slot)
        done_steps, faces, seen = 0, np.zeros(5, np.int64), dict(absent=0, none=0, now=0, several=0, later=0)
        for k in states_of(E):
            if k > done_steps:
                eng.step(k - done_steps)
            done_steps = k
            st = eng.state(raw=True)
            assert int(st["n_steps"].max()) == k
            scenes = ttc_scenes(oracle, st, bbox, scen)
            for horizon in HORIZONS:
                want = ttc_reference(oracle, st, bbox, scen, slot, horizon, scenes)
                want_ego = tuple(a[-R:] for a in want)
                rc, got, frames = _raw(eng, n, True, horizon)
                assert rc == 0 and _guards_intact(*frames)
                assert same(got, want), (k, horizon, _mismatches(got, want, scen, slot))
                rc, ego, frames = _raw(eng, R, False, horizon)
                assert rc == 0 and same(ego, want_ego) and _guards_intact(*frames)
                assert all(a[-R:].tobytes() == b.tobytes() for a, b in zip(got, ego))
                assert got[0][R * E - 1].tobytes() == got[0][R * E].tobytes() == got[0][R * E + 1].tobytes()  # the duplicates
                assert same([t.cpu().numpy() for t in eng.time_to_collision_observers(horizon, torch_out=True)], want)
                assert same([t.cpu().numpy() for t in eng.time_to_collision(horizon, torch_out=True)], want_ego)
                if horizon == 2.5:
                    f, i = want[0][:R * E], want[1][:R * E]
                    seen["absent"] += int((i[:, 1] < 0).sum())
                    seen["none"] += int((i[:, 1] == 0).sum())
                    seen["now"] += int(((i[:, 0] >= 0) & (f[:, 0] == 0.0)).sum())
                    seen["later"] += int((np.isfinite(f[:, 0]) & (f[:, 0] > 0.0) & (f[:, 0] <= 2.5)).sum())
                    seen["several"] += int((i[:, 1] >= 2).sum())
                    faces += np.bincount(i[i[:, 0] >= 0, 2] + 1, minlength=5)
        print(f"{recipe} E={E}: {seen}, faces -1..3 {faces.tolist()}")
        assert (seen["absent"] or (recipe, E) == ("mixed", 3)) and seen["none"] and seen["now"] and seen["later"]
        assert E == 3 or ((faces > 0).all() and seen["several"])
    finally:
        eng.close()


@gpu
def test_a_drivers_ttc_follows_its_driven_velocity(sga, oracle):
    """A driver scene stepped with sg_step_drivers: driver "a" heads for the parked victim, and is accelerated or braked away from
    the 6 m/s of its recording.  Its time to collision is that of the velocity the state holds -- bit for bit the yardstick's on
    the device's state, the closing speed reported is the driven one and not the recorded one -- which a look-ahead along the
    recordings (sg_future_collision) cannot know."""
    E = 8
    scs = DS.batch(E, [[(0, "a"), (2, "b"), (3, "free")], [(0, "a")], [(0, "a"), (2, "b")]], seed=4)
    scen, slot = DS.driver_list(scs)
    acts = DS.actions(len(scen), seed=9)
    acts[:, :, 1] = 0.0  # straight on
    eng = sga.RolloutEngine(len(scs), E, timestep=DS.DT, terminal_conditions=["max_length"])
    try:
        eng.upload(DS.pack(scs))
        eng.set_drivers(scen, slot)
        eng.set_observers(scen, slot)
        eng.reset()
        bbox = np.array([s["bbox"] for s in scs])
        a_rows = [i for i in range(len(scen)) if slot[i] == 0]
        away = 0.0
        for k in range(6):
            eng.step_drivers(acts[k:k + 1], 1)
            st = eng.state(raw=True)
            want = ttc_reference(oracle, st, bbox, scen, slot, 2.5)
            rc, got, frames = _raw(eng, len(scen), True, 2.5)
            assert rc == 0 and same(got, want), (k, _mismatches(got, want, scen, slot))
            for i in a_rows:
                v = float(st["vels"][scen[i], 0, 0])
                away = max(away, abs(v - 6.0))
                assert got[1][i, 0] == DS.VICTIM and got[1][i, 2] == 0  # the victim ahead, met with the front
                assert got[0][i, 2] == -v and 0.0 < got[0][i, 0] < 2.5  # (the victim stands: the relative velocity is minus the driven one)
        assert away > 0.5  # ... which is not the recording's
    finally:
        eng.close()


@gpu
def test_outputs_absent_observers_and_an_empty_list(sga, oracle):
    """HOST and DEVICE outputs are the same bytes; info == NULL is accepted and leaves its buffer alone; poisoned buffers are fully
    overwritten and nothing around them; an absent observer gets -1, -1, -1 and zeros; an empty observer list writes nothing, with
    NULL feat too; device outputs queued right behind a step see the stepped state."""
    import torch

    E = 48
    scs = B.batch("yard", E)
    R = len(scs)
    eng, bbox = _yard_engine(sga, scs, E)
    try:
        # no observers set: nothing is written, NULL feat is fine
        rc, _, frames = _raw(eng, 4, True, 2.5)
        assert rc == 0 and _untouched(*frames)
        assert eng.lib.sg_time_to_collision_observers(eng.h, 2.5, None, None, 0) == 0
        assert eng.lib.sg_time_to_collision_observers(eng.h, 2.5, None, None, 1) == 0
        assert [a.shape for a in eng.time_to_collision_observers(2.5)] == [(0, NFEAT), (0, NINFO)]
        scen, slot = _observers(R, E)
        n = len(scen)
        eng.set_observers(scen, slot)
        eng.step(12)
        st = eng.state(raw=True)
        want = ttc_reference(oracle, st, bbox, scen, slot, 2.5)
        absent = ~st["present"][scen, slot]
        assert absent.any() and (want[1][absent] == -1).all() and not want[0][absent].any() and not np.signbit(want[0][absent]).any()
        rc, got, frames = _raw(eng, n, True, 2.5)
        assert rc == 0 and same(got, want) and _guards_intact(*frames)
        rc, (f, i), frames = _raw(eng, n, True, 2.5, want_info=False)
        assert rc == 0 and f.tobytes() == want[0].tobytes() and _untouched(frames[1]) and _guards_intact(*frames)
        rc, (f, i), frames = _raw(eng, R, False, 2.5, want_info=False)
        assert rc == 0 and f.tobytes() == want[0][-R:].tobytes() and _untouched(frames[1])
        # raw device outputs into poisoned, guarded buffers, queued right behind a step
        sizes = (n * NFEAT * 8, n * NINFO * 4)
        d = [torch.full((b + 2 * GUARD,), 0xCC, dtype=torch.uint8, device="cuda:0") for b in sizes]
        torch.cuda.synchronize()
        assert eng.lib.sg_step(eng.h, 3, None, 0) == 0
        assert eng.lib.sg_time_to_collision_observers(eng.h, 2.5, *[t.data_ptr() + GUARD for t in d], 1) == 0
        assert eng.lib.sg_synchronize(eng.h) == 0
        st2 = eng.state(raw=True)
        want2 = ttc_reference(oracle, st2, bbox, scen, slot, 2.5)
        back = [t.cpu().numpy() for t in d]
        got2 = (back[0][GUARD:-GUARD].view(np.float64).reshape(n, NFEAT), back[1][GUARD:-GUARD].view(np.int32).reshape(n, NINFO))
        assert same(got2, want2) and not same(want2, want) and _guards_intact(*back)
        rc, host2, frames = _raw(eng, n, True, 2.5)
        assert rc == 0 and same(host2, got2)
        dev_only = torch.full((sizes[0],), 0xCC, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert eng.lib.sg_time_to_collision_observers(eng.h, 2.5, dev_only.data_ptr(), None, 1) == 0 and eng.lib.sg_synchronize(eng.h) == 0
        assert dev_only.cpu().numpy().tobytes() == want2[0].tobytes()
        eng.set_observers([], [])
        rc, _, frames = _raw(eng, 4, True, 2.5)
        assert rc == 0 and _untouched(*frames)
    finally:
        eng.close()


@gpu
def test_refusals(sga, oracle):
    """SG_ERR_STATE before sg_upload; SG_ERR_INVALID for a horizon that is NaN or negative and for NULL feat when there is something
    to write -- each with a message that names the call, nothing written into sentinel-filled buffers, and the next valid call
    works."""
    E = 3
    scs = B.batch("yard", E)
    R = len(scs)
    fresh = sga.RolloutEngine(R, E, timestep=B.DT)
    for observers, name in zip((False, True), NEW_SYMBOLS):
        rc, _, frames = _raw(fresh, R, observers, 2.5)
        assert rc == SG_ERR_STATE and _untouched(*frames)
        assert fresh.lib.sg_last_error(fresh.h).decode().startswith(name + ":")
    fresh.close()
    eng, bbox = _yard_engine(sga, scs, E)
    try:
        eng.step(5)
        st = eng.state(raw=True)
        obs = ([0, 1, 2, 2], [1, 2, 1, 1])
        eng.set_observers(*obs)
        for observers, name, n in ((False, NEW_SYMBOLS[0], R), (True, NEW_SYMBOLS[1], 4)):
            lists = (np.arange(R), np.zeros(R, int)) if not observers else obs
            for dev in (0, 1):
                for horizon in (float("nan"), -1.0, -INF, float(np.nextafter(0.0, -1.0))):
                    rc, _, frames = _raw(eng, n, observers, horizon, device=dev)
                    assert rc == SG_ERR_INVALID and _untouched(*frames), (name, horizon)
                    assert eng.lib.sg_last_error(eng.h).decode().startswith(name + ":")
                (info, f1) = _cc((n, NINFO), np.int32)
                rc = getattr(eng.lib, name)(eng.h, 2.5, None, info.ctypes.data if not dev else None, dev)
                assert rc == SG_ERR_INVALID and _untouched(f1), (name, dev)
                assert eng.lib.sg_last_error(eng.h).decode().startswith(name + ":")
                rc, got, frames = _raw(eng, n, observers, 2.5)
                assert rc == 0 and same(got, ttc_reference(oracle, st, bbox, *lists, 2.5)) and _guards_intact(*frames)
        assert _raw(eng, R, False, -0.0)[0] == 0  # (-0.0 is not negative)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------- GPU: the Python layers
def _short_driver_scenes(E, lists, roles):
    """The driver scenes with scenarios 1 and 2 cut to 1.25 s: they end (max_length) and start anew within a run."""
    scs = DS.batch(E, [list(zip(l, r)) for l, r in zip(lists, roles)], seed=4)
    for sc in scs[1:3]:
        for e in range(E):
            a, b = sc["knot_off"][e], sc["knot_off"][e + 1]
            if b - a == 2:
                sc["knots"][b - 1, 1:3] = sc["knots"][a, 1:3] + (sc["knots"][b - 1, 1:3] - sc["knots"][a, 1:3]) * (1.25 - sc["knots"][a, 0]) / (
                    sc["knots"][b - 1, 0] - sc["knots"][a, 0])
                sc["knots"][b - 1, 0] = 1.25
        sc["length"] = float(sc["knots"][:, 0].max())
    return scs


@gpu
@pytest.mark.parametrize("device_tick", (False, True), ids=("host-tick", "device-tick"))
def test_vector_env_driver_ttc(sga, oracle, device_tick):
    """VectorScenarioEnv(drivers=..., driver_ttc=2.5) on the driver scenes, two of them so short that they restart within the run:
    after reset() and after every step info["driver_ttc"] / ["driver_ttc_info"] are, byte for byte, a separate
    time_to_collision_observers call on the state the environment holds then -- the one behind the auto-reset -- and the
    yardstick on it; obs, reward, done and the rest of info are those of a twin without driver_ttc; an environment whose caller has
    an observer list of its own reports the same rows and keeps its list; driver "a" sees the victim come closer."""
    import torch

    E = 8
    lists = [[0, 2, 3], [0], [], [3, 0], [2], [0, 2, 3]]
    roles = [["a", "b", "free"], ["a"], [], ["a", "b"], ["a"], ["a", "b", "c"]]
    scs = _short_driver_scenes(E, lists, roles)
    objs = _driver_objects(scs)
    scen, slot = DS.driver_list(scs)
    nd = len(scen)
    bbox = np.array([s["bbox"] for s in scs])
    acts = DS.actions(nd, seed=9)
    acts[:, :, 1] *= 0.02
    kw = dict(timestep=DS.DT, n=8, terminal_conditions=["max_length"], max_steer=0.9, max_accel=5.0, drivers=lists, torch_obs=device_tick,
              device_tick=device_tick)
    with pytest.raises(ValueError):
        sga.VectorScenarioEnv(objs, timestep=DS.DT, n=8, driver_ttc=2.5)
    env, twin, own = (sga.VectorScenarioEnv(objs, driver_ttc=2.5, **kw), sga.VectorScenarioEnv(objs, **kw),
                      sga.VectorScenarioEnv(objs, driver_ttc=2.5, **kw))
    own_lists = [[1], [], [4, 4], [], [0], []]
    host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)  # noqa: E731

    def check(e, info, k):
        st = e.engine.state(raw=True)
        sep = e.engine.time_to_collision_observers(2.5) if e is env else None  # (env's observers are its drivers)
        got = (host(info["driver_ttc"]), host(info["driver_ttc_info"]))
        assert got[0].shape == (nd, NFEAT) and got[1].shape == (nd, NINFO) and got[1].dtype == np.int32
        if sep is not None:
            assert got[0].tobytes() == sep[0].tobytes() and got[1].tobytes() == sep[1].tobytes(), k
        assert same(got, ttc_reference(oracle, st, bbox, scen, slot, 2.5)), k
        return st, got

    first = env.reset()
    assert np.array_equal(host(first), host(twin.reset())) and twin.reset_info == {}
    own.reset()
    own.set_observers(own_lists)
    check(env, env.reset_info, "reset")
    restarted, closing = np.zeros(len(scs), bool), []
    for k in range(24):
        a = torch.as_tensor(acts[k], device="cuda:0") if device_tick else acts[k]
        obs, reward, done, info = env.step(a)
        obs2, reward2, done2, info2 = twin.step(a)
        _, _, _, info3 = own.step(a)
        if device_tick:
            assert all(isinstance(info[q], torch.Tensor) and info[q].is_cuda for q in ("driver_ttc", "driver_ttc_info"))
        assert set(info) == set(info2) | {"driver_ttc", "driver_ttc_info"} and set(info3) == set(info)
        assert np.array_equal(host(obs), host(obs2)) and host(reward).tobytes() == host(reward2).tobytes() and np.array_equal(host(done), host(done2))
        assert all(host(info[q]).tobytes() == host(info2[q]).tobytes() for q in info2)
        st, got = check(env, info, k)
        check(own, info3, k)
        assert host(info3["driver_ttc"]).tobytes() == got[0].tobytes() and host(info3["driver_ttc_info"]).tobytes() == got[1].tobytes()
        assert [list(host(x)) for x in own.time_to_collision_observers(2.5)[2:]] == [[i for i, s in enumerate(own_lists) for _ in s], [q for s in own_lists for q in s]]
        d = host(done)
        assert (st["n_steps"][d] == 0).all()  # the rows describe the state behind the auto-reset
        restarted |= d
        if got[1][0, 0] == DS.VICTIM:
            closing.append(float(got[0][0, 0]))
    assert restarted[1:3].all() and not restarted[[0, 3, 4, 5]].any()
    assert len(closing) >= 3 and closing[0] > closing[-1]
    ego = env.time_to_collision(2.5)
    assert same([host(x) for x in ego], ttc_reference(oracle, env.engine.state(raw=True), bbox, np.arange(len(scs)), np.zeros(len(scs), int), 2.5))
    for e in (env, twin, own):
        e.close()


@gpu
def test_state_time_to_collision_and_the_all_slots_form(sga, oracle):
    """State.time_to_collision through ScenarioGym names the right Entity objects, for the ego and for any entity, and
    BatchedScenarioGym.time_to_collision gives every slot's rows at once."""
    E = 8
    scs = DS.batch(E, [[(0, "a"), (2, "b"), (3, "free")]], seed=4)
    for sc in scs:
        sc["kind"][:] = np.where(sc["kind"] == DS.KIND_AGENT_EXTERNAL, DS.KIND_REPLAY, sc["kind"])
    objs = _driver_objects(scs)
    bbox = np.array([s["bbox"] for s in scs])
    gym = sga.ScenarioGym(timestep=DS.DT, terminal_conditions=[])
    gym.set_scenario(objs[0])
    ents = gym.state.scenario.entities
    threats = set()
    for k in range(16):
        gym.step()
        st = gym._b.engine.state(raw=True)
        for horizon in (1.0, INF):
            feat, info = ttc_reference(oracle, st, bbox, np.zeros(E, int), np.arange(E), horizon)
            whole = gym._b.time_to_collision(horizon)
            assert same(tuple(x[0] for x in whole), (feat, info))
            for j in (0, 2, DS.VICTIM, 5):
                s = gym.state.time_to_collision(ents[j], horizon=horizon) if j else gym.state.time_to_collision(horizon=horizon)
                assert isinstance(s, sga.TimeToCollision)
                assert (s.ttc, s.until, s.n_contacts, s.face) == (feat[j, 0], feat[j, 1], info[j, 1], info[j, 2])
                assert s.rel_velocity.tobytes() == feat[j, 2:4].tobytes()
                assert s.entity is (ents[info[j, 0]] if info[j, 0] >= 0 else None)
                threats.add((j, int(info[j, 0])))
    # "a" meets the victim first and stays in it; the victim and the oncoming "b" both see "a"; the far entity sees nobody
    assert (0, DS.VICTIM) in threats and (DS.VICTIM, 0) in threats and (2, 0) in threats and (5, -1) in threats
    gym.close()


@gpu
def test_min_time_to_collision_metric(sga, reference_inputs):
    """MinTimeToCollision(5) on one OpenSCENARIO file of the reference's test inputs: after rollout() it holds the smallest ego ttc over the reset state and every
    stepped state, and the time of the first state that had it -- the minimum of the per-step ego rows of a second gym stepped by
    hand."""
    import glob

    for path in sorted(glob.glob(os.path.join(reference_inputs, "Scenarios", "*.xosc"))):  # the first file whose ego meets anybody within 5 s
        metric = sga.MinTimeToCollision(5.0)
        gym = sga.ScenarioGym(timestep=0.1, metrics=[metric])
        gym.load_scenario(path)
        gym.rollout()
        got = gym.get_metrics().get("min_time_to_collision")
        gym.close()
        if got[0] < INF:
            break
    assert got[0] < INF and got[1] is not None
    plain = sga.ScenarioGym(timestep=0.1)
    plain.load_scenario(path)
    rows = [(plain.state.time_to_collision(horizon=5.0), plain.state.t)]
    while not plain.state.is_done:
        plain.step()
        rows.append((plain.state.time_to_collision(horizon=5.0), plain.state.t))
    plain.close()
    assert len(rows) > 10 and all(isinstance(r, sga.TimeToCollision) for r, _ in rows)
    met = [(r.ttc, t) for r, t in rows if r.n_contacts > 0]
    print(f"{os.path.basename(path)}: {len(rows)} states, {len(met)} with a threat within 5 s, metric {got}")
    want = min(met, key=lambda x: x[0])  # (min keeps the first of equals)
    assert got == want and metric.get_state() == want
