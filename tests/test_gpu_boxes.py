"""Device collisions -- and every other device reader of a state block's box fields -- on MIXED box sizes and off-axis box
centres (tests/box_scenes.py), through the C ABI.  Every comparison is exact equality.

Until here every scene the device was given had one box per tile (the car, the lattice box, the pedestrian) and center_y = 0,
so the layer of the collision pass that only matters when boxes differ changed no output: the reduction of the tile's largest
radius and centre offset over lanes and wavefronts (rmax / omax / omax_ped -> rad_thr, trig_eps, nbr_thr, the stripe cell
size), tile_centre's bcy terms, which component of `half` is the length, REFINE / hetero, wide_collide_kernel's s_rmax.

* the 10,000 labelled OBB pairs of collision.npz (random widths, lengths and centres; exact rational labels), one scenario of
  two static entities each, on the device;
* yard scenes of every kernel family x tile shape: collision rows of EVERY scenario after EVERY step against the oracle (which
  tests/test_boxes_cpu.py holds against the exact predicate on these very scenes), then final state, metric rows and events
  (oracle/check.py compare_final), for the RSS family the four RSSDistances records after every step;
* the same yards 3e4 .. 7.5e5 m from the origin: with a giant in every tile the stripe cell is 13 - 20 m, so the scenarios at
  2e5 and 7.5e5 m (four of six) are beyond 4000 cells and take the all-pairs fallback with the giant's reach, those at 3e4 m
  stay on the stripe masks at large cell coordinates (nothing reports which broad phase ran: this follows from tile_centre);
* pairs of static entities with a zero-width or a zero-length box, labelled by the exact predicate;
* entity raster, look-ahead detector and the collision classes of the events on a yard scene.

CASES steers the dispatcher with the knobs of tests/test_gpu_variants.py and asserts sg_last_kernel() after every call.
Families whose kernels do several steps per launch by design (the table path, the time-sliced path, the crowd kernel with
riders) are checked by PREFIX: sg_rollout(k) from the reset for every k, rows after the k-th step -- each call a launch of
that family, chunk boundaries and skipped collision passes included; the others step by step (sg_step(1)).  ONE step is not
compared: the time-sliced path takes calls of two steps and more, so the slice cases start at k = 2 and the rows after their
first step are seen by no call of rollout_kernel_slice (the same scenes' first step is compared in the tab_rows cases)."""
import numpy as np
import pytest

import box_scenes as B
import test_gpu_variants as V
from conftest import load_golden
from test_boxes_cpu import SCENES
from test_gpu_variants import sga  # noqa: F401  (the fixture)

gpu = pytest.mark.gpu
SHAPE = {E: (G, WV) for E, G, WV, _ in V.SHAPES}
EV_CAP = 256


def _case(family, recipe, E, expect, ego="sparse", far=False, tuning=V.NO_TAB, env=None, rss=False, road=False, slicing=False,
          prefix=False):
    return dict(id=f"{family}-{recipe}-E{E}" + ("-far" if far else ""), family=family, scene=(recipe, E, ego, far), expect=expect,
                tuning=tuning, env=env or {}, rss=rss, road=road, slicing=slicing, prefix=prefix)


def _cases():
    out = []
    for E, (G, WV) in SHAPE.items():  # every tile shape
        out.append(_case("plain", "yard", E, f"sg::rollout_kernel<{G}, {WV}, false, false>"))
    for E in (24, 48, 200):  # (one wavefront: no controlled lane, else the planar table kernel runs)
        G, WV = SHAPE[E]
        out.append(_case("tab_rows", "yard", E, f"sg::rollout_kernel<{G}, {WV}, false, true>",
                         ego="replay" if WV == 1 else "sparse", tuning=V.TAB, prefix=True))
    for E in (6, 24, 48):
        out.append(_case("tab_planar", "yard", E, f"sg::rollout_kernel_tab_planar<{SHAPE[E][0]}>", tuning=V.TAB,
                         env=dict(SG_QUEUE="0"), prefix=True))
    for E in (3, 12, 48):
        out.append(_case("tabq_planar", "yard", E, f"sg::rollout_kernel_tabq_planar<{SHAPE[E][0]}>", tuning=V.TAB, prefix=True))
    for E in (6, 24, 48):
        out.append(_case("slice", "yard", E, f"sg::rollout_kernel_slice<{SHAPE[E][0]}>", ego="replay", tuning={}, slicing="always",
                         prefix=True))
    for E in (12, 48, 300):
        out.append(_case("road", "yard", E, "sg::rollout_kernel_road<%d, %d>" % SHAPE[E], road=True))
    for E in (6, 48, 100):
        out.append(_case("rss", "yard", E, "sg::rollout_kernel_rss<%d, %d>" % SHAPE[E], rss=True))
    for E in (12, 48, 200, 300):  # vehicles of every class among pedestrian agents: REFINE / hetero
        G, WV = SHAPE[E]
        out.append(_case("ped", "mixed", E, f"sg::rollout_kernel<{max(G, 16)}, {WV}, true, false>"))
    for E in (48, 100, 200):
        out.append(_case("crowd_riders", "mixed", E, f"sg::rollout_kernel_crowd_riders<{SHAPE[E][1]}>", tuning=V.TAB, prefix=True))
    out += [_case("wide", "yard", 600, V.WIDE), _case("wide", "yard", 1100, V.WIDE), _case("wide", "mixed", 600, V.WIDE)]
    for E in (12, 100):  # far from the origin: the all-pairs fallback
        G, WV = SHAPE[E]
        out.append(_case("plain", "yard", E, f"sg::rollout_kernel<{G}, {WV}, false, false>", far=True))
        out.append(_case("ped", "mixed", E, f"sg::rollout_kernel<{max(G, 16)}, {WV}, true, false>", far=True))
    return out


CASES = _cases()


def test_scenes_are_checked_on_the_cpu():
    """Every batch uploaded here is a scene of tests/test_boxes_cpu.py (oracle against the exact predicate, decisive pairs), and
    the cases cover what they are meant to: every family at a narrow tile, at 64 lanes and at several wavefronts where it has
    them, every tile shape of test_gpu_variants.SHAPES, both widths of the multi-kernel step."""
    assert {c["scene"] for c in CASES} | {("yard", 12, "sparse", False), ("yard", 300, "sparse", False)} == set(SCENES)
    assert len({c["id"] for c in CASES}) == len(CASES)
    fam = {}
    for c in CASES:
        if not c["scene"][3]:
            fam.setdefault(c["family"], set()).add(c["scene"][1])
    assert set(fam) == {"plain", "tab_rows", "tab_planar", "tabq_planar", "slice", "road", "rss", "ped", "crowd_riders", "wide"}
    assert fam["plain"] == set(SHAPE) and fam["wide"] == {600, 1100}
    for f, Es in fam.items():
        lanes = {SHAPE[E][0] * SHAPE[E][1] for E in Es if E in SHAPE}
        if f in ("tab_planar", "tabq_planar", "slice"):  # one wavefront at the most
            assert min(lanes) < 64 and 64 in lanes and len(lanes) >= 3, f
        elif f == "crowd_riders":                          # 64-lane tiles only
            assert lanes == {64, 128, 256}, f
        elif f != "wide":
            assert min(lanes) < 64 and 64 in lanes and max(lanes) > 64, f


# ------------------------------------------------------------------------------------------------ helpers
def _pack(scs):
    from scenario_gym_amd.engine import DEFAULT_CTRL
    from scenario_gym_amd.packing import pack_arrays

    return pack_arrays(scs, kinds=[s["kind"] for s in scs], ctrls=[B.ctrl_rows(s, DEFAULT_CTRL) for s in scs])


_NETS = {}
_REF = {}


def _road_of(scene, road):
    """(networks, net_of_scenario) of a scene under ego_off_road: the random polygons of test_gpu_variants (they cover the
    yard: those egos stay on the road), for scenarios 1, 5, .. a network of one 2 m square of road around the ego's first
    knot, which the ego leaves during the run, and one scenario in four without a network."""
    if not road:
        return None, None
    if "nets" not in _NETS:
        _NETS["nets"] = V._nets(11)
    nets = list(_NETS["nets"])
    scs = B.batch(*scene)
    net_of = np.array([-1 if r % 4 == 3 else r % len(nets) for r in range(len(scs))], np.int32)
    for r in range(1, len(scs), 4):
        c = scs[r]["knots"][0, 1:3]
        net_of[r] = len(nets)
        nets.append(dict(ring_off=np.arange(2), vert_off=np.array([0, 4]), layers=np.ones(1, int),
                         verts=c + np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])))
    return nets, net_of


def _reference(O, scene, road, terminal_mask):
    """The oracle's run of every scenario of a scene (every step recorded), computed once per (scene, road)."""
    key = (scene, road)
    if key not in _REF:
        nets, net_of = _road_of(scene, road)
        steps = B.steps_of(scene[1])
        _REF[key] = [B.oracle_rollout(O, sc, steps, event_cap=EV_CAP, terminal_mask=terminal_mask, force_steps=True,
                                      road=None if nets is None or net_of[r] < 0 else nets[net_of[r]])
                     for r, sc in enumerate(B.batch(*scene))]
    return _REF[key]


def _rows(coll_r, o_coll_k):
    """Device collision rows [E] / [E][W] of one scenario against the oracle's [E][W] of one step."""
    E, W = o_coll_k.shape
    return np.array_equal(np.asarray(coll_r).reshape(len(coll_r), -1)[:E, :W], o_coll_k)


# ------------------------------------------------------------------------------------------------ the labelled pairs
@gpu
def test_labelled_pairs_on_the_device(sga):
    """The 10,000 OBB pairs of collision.npz -- random widths, lengths, center_x AND center_y, labelled by exact rational
    SAT -- as 10,000 scenarios of two static entities at the fixture's own poses (nothing is translated: the labels hold).
    After a step (static entities stay where they were uploaded; the poses are checked) bit 1 of entity 0's row and bit 0 of
    entity 1's row equal the label, for every pair."""
    from scenario_gym_amd.packing import pack_arrays

    g = load_golden("collision")
    lab = g["pairs/intersects"].astype(bool)
    n = len(lab)
    scs = []
    for pa, pb, ba, bb in zip(g["pairs/pose_a"], g["pairs/pose_b"], g["pairs/box_a"], g["pairs/box_b"]):
        scs.append(dict(knot_off=np.array([0, 1, 2]), knots=np.array([[0.0, *pa], [0.0, *pb]]), bbox=np.array([ba, bb]),
                        etype=np.zeros(2, np.int32), ego=0, t0=0.0, length=1.0))
    assert (g["pairs/box_a"][:, 3] != 0).mean() > 0.9 and len({tuple(b) for b in g["pairs/box_a"]}) > n // 2
    eng = sga.RolloutEngine(n, 2, timestep=0.1)
    try:
        eng.upload(pack_arrays(scs))
        eng.step(1)
        st = eng.state()
    finally:
        eng.close()
    assert np.array_equal(st["poses"][:, 0], g["pairs/pose_a"]) and np.array_equal(st["poses"][:, 1], g["pairs/pose_b"])
    coll = np.asarray(st["coll"]).reshape(n, 2).astype(np.uint64)
    wrong = np.nonzero((coll[:, 0] != lab.astype(np.uint64) * np.uint64(2)) | (coll[:, 1] != lab.astype(np.uint64)))[0]
    assert len(wrong) == 0, (len(wrong), wrong[:10].tolist(), coll[wrong[:10]].tolist(), lab[wrong[:10]].tolist())
    assert 0.2 < lab.mean() < 0.5


@gpu
def test_zero_extent_pairs_on_the_device(sga, oracle):
    """4,000 scenarios of two static entities, the first with a zero-width or a zero-length box (box_scenes.ZERO_EXTENT), the
    second with one of those or an ordinary box, at continuous random poses; the label of a pair is quads_meet_exact on the
    oracle's corners (the exact rational predicate; test_boxes_cpu.py holds the oracle to it on the same construction).
    Bit 1 of entity 0's row and bit 0 of entity 1's row equal the label, for every pair."""
    from scenario_gym_amd.packing import pack_arrays

    rng = np.random.default_rng(11)
    boxes = [np.array(b) for b in B.ZERO_EXTENT + (B.CAR, B.SKEW[1], B.PED_BOX, B.LORRY)]
    n = 4000
    scs, lab = [], np.zeros(n, bool)
    for q in range(n):
        ba, bb = boxes[q % 2], boxes[rng.integers(len(boxes))]
        pa, pb = (np.array([*rng.uniform(-3, 3, 2), 0.0, rng.uniform(-3.2, 3.2), 0.0, 0.0]) for _ in range(2))
        lab[q] = B.quads_meet_exact(oracle.corners(pa, ba), oracle.corners(pb, bb))
        scs.append(dict(knot_off=np.array([0, 1, 2]), knots=np.array([[0.0, *pa], [0.0, *pb]]), bbox=np.array([ba, bb]),
                        etype=np.zeros(2, np.int32), ego=0, t0=0.0, length=1.0))
    eng = sga.RolloutEngine(n, 2, timestep=0.1)
    try:
        eng.upload(pack_arrays(scs))
        eng.step(1)
        st = eng.state()
    finally:
        eng.close()
    coll = np.asarray(st["coll"]).reshape(n, 2).astype(np.uint64)
    wrong = np.nonzero((coll[:, 0] != lab.astype(np.uint64) * np.uint64(2)) | (coll[:, 1] != lab.astype(np.uint64)))[0]
    assert len(wrong) == 0, (len(wrong), wrong[:10].tolist(), coll[wrong[:10]].tolist(), lab[wrong[:10]].tolist())
    assert 0.1 < lab.mean() < 0.7


# ------------------------------------------------------------------------------------------------ yards, every step
@gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_yard_collisions_every_step(sga, oracle, monkeypatch, case):
    """One case of CASES: the dispatcher names the family after every call; collision rows of every scenario after every step
    equal the oracle's (RSS family: the RSSDistances codes and safe distances too); after the last step final state, metric
    rows and events (t, other, collision class) equal the oracle's by compare_final, and the RSS flags."""
    from oracle import check

    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    scene = case["scene"]
    scs = B.batch(*scene)
    R, E = len(scs), scene[1]
    steps = B.steps_of(E)
    term = ["max_length", "ego_off_road"] if case["road"] else ["max_length"]
    ref = _reference(oracle, scene, case["road"], sga.engine.terminal_mask(term))
    rss_ref = [oracle.rss_rollout(o, sc["bbox"], 0) for o, sc in zip(ref, scs)] if case["rss"] else None
    assert all(o["n_steps"] == steps for o in ref)
    if case["road"]:  # some ego with a network under it stays on the road, some ego leaves it: ego_off_road does fire
        net_of = _road_of(scene, True)[1]
        assert {bool(o["is_done"]) for o, n in zip(ref, net_of) if n >= 0} == {False, True}
    packed = _pack(scs)
    eng = sga.RolloutEngine(R, E, timestep=B.DT, terminal_conditions=term, event_capacity=EV_CAP)
    n_bits = n_rss = 0
    try:
        if case["tuning"]:
            eng.set_tuning(**case["tuning"])
        eng.set_slicing(case["slicing"])
        eng.set_rss(case["rss"])
        eng.upload(packed)
        nets, net_of = _road_of(scene, case["road"])
        if nets is not None:
            eng.set_road_networks(nets, net_of)
        for k in range(2 if case["slicing"] else 1, steps + 1):  # (the time-sliced path takes calls of two steps and more)
            if case["prefix"]:
                eng.rollout(k)
            else:
                eng.step(1)
            assert eng.last_kernel() == case["expect"], (k, eng.last_kernel())
            st = eng.state()
            bad = [r for r in range(R) if not _rows(st["coll"][r], ref[r]["coll"][k])]
            assert not bad, f"collision rows after step {k}: scenarios {bad}"
            n_bits += int(sum(np.unpackbits(ref[r]["coll"][k].view(np.uint8)).sum() for r in range(R)))
            if case["rss"]:
                rs = eng.rss()
                for r in range(R):
                    assert np.array_equal(rs[2][r, :E], rss_ref[r]["code"][k]), ("rss codes", k, r)
                    assert check._bits(rs[3][r, :E], rss_ref[r]["safe"][k]), ("rss safe distances", k, r)
                    n_rss += int((rss_ref[r]["code"][k] > 0).sum())
        st = eng.state()
        rows, events = eng.metrics()
        bad = {}
        for r in range(R):
            b = check.compare_final(st, rows, events, r, ref[r], E, event_cap=EV_CAP, kind=packed.kind[r * E:(r + 1) * E])
            if case["rss"]:
                rs = eng.rss()
                if bool(rs[0][r]) != bool(rss_ref[r]["safe_longitudinal"]) or bool(rs[1][r]) != bool(rss_ref[r]["safe_lateral"]):
                    b.append("rss_flags")
            if b:
                bad[r] = b
        assert not bad, bad
    finally:
        eng.close()
    assert n_bits > 10 * steps  # (the yards do collide throughout)
    assert not case["rss"] or n_rss > 0
    assert sum(o["n_events"] for o in ref) > 0


# ------------------------------------------------------------------------------------------------ observations
@gpu
@pytest.mark.parametrize("E", [12, 300])
def test_observations_on_a_yard(sga, oracle, E):
    """The other device readers of the box fields, on a yard of mixed boxes: the entity raster (sg_raster_entities for the ego,
    sg_raster_map_observers' entity layer for observers that include the giant and a box whose reference point lies outside
    it, and zero-extent boxes) against oracle.raster_entities, and the look-ahead detector (sg_future_collision / _observers) against
    oracle.future_collision, at the reset and after 12 and 40 steps; then the collision classes of the events
    (classify_events_kernel) against the oracle's classification.  That last one is DEVICE AGAINST ORACLE only: the oracle's
    classifier is pinned on the reference for the car box alone (collision_types.npz)."""
    scene = ("yard", E, "sparse", False)
    scs = B.batch(*scene)
    R, steps = len(scs), B.steps_of(E)
    ref = _reference(oracle, scene, False, sga.engine.terminal_mask(["max_length"]))
    obs = []
    for r, sc in enumerate(scs):
        outside = [e for e in range(1, E) if tuple(sc["bbox"][e]) in B.OUTSIDE]
        skew = [e for e in range(1, E) if tuple(sc["bbox"][e]) in B.SKEW]
        flat = [e for e in range(1, E) if tuple(sc["bbox"][e]) in B.ZERO_EXTENT]
        obs += [(r, e) for e in dict.fromkeys([0, sc["giant"]] + outside[:2] + skew[:1] + flat[:2] + [E // 2])]
    assert any(tuple(scs[r]["bbox"][e]) in B.OUTSIDE for r, e in obs) and any(tuple(scs[r]["bbox"][e]) in B.ZERO_EXTENT for r, e in obs)
    eng = sga.RolloutEngine(R, E, timestep=B.DT, event_capacity=EV_CAP)
    cells = flags = 0
    try:
        eng.set_tuning(**V.NO_TAB)
        eng.upload(_pack(scs))
        eng.set_observers([o[0] for o in obs], [o[1] for o in obs])
        for n_adv in (0, 12, steps - 12):
            if n_adv:
                eng.step(n_adv)
            st = eng.state()
            for w, h, nw, nh in ((30.0, 30.0, 24, 24), (44.0, 20.0, 33, 13)):
                ego = eng.raster_entities(w, h, nw, nh)
                got = eng.raster_map_observers([0], w, h, nw, nh)[:, 0]
                for r, sc in enumerate(scs):
                    assert np.array_equal(ego[r], oracle.raster_entities(st["poses"][r, :E], sc["bbox"], 0, w, h, nw, nh)), (n_adv, r)
                for j, (r, e) in enumerate(obs):
                    want = oracle.raster_entities(st["poses"][r, :E], scs[r]["bbox"], e, w, h, nw, nh)
                    assert np.array_equal(got[j], want), (n_adv, r, e, int((got[j] != want).sum()))
                    cells += int(want.sum())
            for horizon, n in ((1.5, 10), (0.4, 3)):
                ego = eng.future_collision(horizon, n)
                got = eng.future_collision_observers(horizon, n)
                for r, sc in enumerate(scs):
                    want = oracle.future_collision(sc["knot_off"], sc["knots"], sc["bbox"], sc["kind"], 0, st["t"][r], horizon, n)
                    assert bool(ego[r]) == want, (n_adv, r, horizon)
                for j, (r, e) in enumerate(obs):
                    sc = scs[r]
                    want = oracle.future_collision(sc["knot_off"], sc["knots"], sc["bbox"], sc["kind"], e, st["t"][r], horizon, n)
                    assert bool(got[j]) == want, (n_adv, r, e, horizon)
                    flags += int(want) + 1000 * int(not want)
        rows, events = eng.metrics()
    finally:
        eng.close()
    assert cells > 200 and flags % 1000 > 0 and flags // 1000 > 0
    types = set()
    for r in range(R):
        ev = events[events["scenario"] == r]
        m = min(int(ref[r]["n_events"]), EV_CAP)
        assert len(ev) == m and np.array_equal(ev["other"], ref[r]["ev_other"][:m]) and np.array_equal(ev["t"], ref[r]["ev_t"][:m]), r
        assert np.array_equal(ev["type"], ref[r]["ev_type"][:m]), (r, ev["type"].tolist(), ref[r]["ev_type"][:m].tolist())
        types |= set(ev["type"].tolist())
    assert len(types) >= 2, types
