"""The replay interpolant on per-entity knot times (tests/knot_scenes.py), on the CPU: the yardstick of
tests/test_gpu_knot_times.py.

* the oracle reproduces tests/golden/knots.npz -- the real reference on small editions of every family (ScenarioGym rollouts
  with replay and PID egos, both `persist` values, dt 0.1 and 1/30; BatchReplayEntity.step at the clock's times) -- and the
  fixture regenerates byte for byte where the reference is at hand;
* on the full-size scenes of the device tests the replayed poses and presence of oracle.rollout equal
  knot_scenes.batch_reference (the reference's two interp1d stages restated in numpy) at clock(...)[1:], bit for bit, and
  batch_reference equals scipy's interp1d itself where scipy imports;
* the scenes reach what they are for (knot_scenes.coverage): steps ON union rows, entities that enter and leave ON a step,
  several rows per step, thousands of rows, rows one ulp apart, collisions -- conditions on the inputs, asserted on the very
  scenes the GPU tests upload.
"""
import os
import sys

import numpy as np
import pytest

import knot_scenes as KS
from conftest import GOLDEN, ROOT, bits_equal, load_golden

DT = 0.1
T = 40
T_LONG = 60
EV_CAP = 256

# The scenes of the device tests: name -> knot_scenes.batch arguments.  One set per family (the `long` family has its own).
SHAPES = {
    "E6":        dict(E=6, R=12, ego="sparse"),                 # PID egos in every fourth scenario (the table kernels' lanes)
    "E6_flat":   dict(E=6, R=12, ego="sparse", zpr="none"),     # ... without z / pitch / roll: the planar kernels
    "E6_replay": dict(E=6, R=12, ego="replay"),                 # nothing controlled: the time-sliced kernel without a table
    "E48":       dict(E=48, R=6, ego="pid"),
    "E48_replay": dict(E=48, R=6, ego="replay"),
    "E100":      dict(E=100, R=4, ego="pid"),
    "E300":      dict(E=300, R=3, ego="vehicle"),
    "crowd":     dict(E=48, R=4, ego="pid", crowd=True),         # replay riders and a PID car among pedestrian agents
    "wide":      dict(E=600, R=2, ego="pid", K=8),
}
KNOT_FAMILIES = ("ragged", "clock", "twins", "offset")
SCENES = {(f, s): dict(family=f, steps=T, dt=DT, **kw) for f in KNOT_FAMILIES for s, kw in SHAPES.items()}
for s in ("E6", "E6_flat", "E6_replay"):  # (five replayed entities: more knots each, so that most steps meet one)
    SCENES[("clock", s)]["K"] = 40
    SCENES[("ragged", s)]["K"] = 120  # (... and a knot crossing in every step, the PID ego's own included)
SCENES[("ragged", "crowd")]["K"] = 16  # (four in ten are pedestrian agents, outside the batch interpolant)
SCENES[("long", "E64")] = dict(family="long", E=64, R=4, ego="sparse", steps=T_LONG, dt=DT)
SCENES[("long", "E64_replay")] = dict(family="long", E=64, R=4, ego="replay", steps=T_LONG, dt=DT)
SCENES[("long", "E64_flat")] = dict(family="long", E=64, R=4, ego="sparse", zpr="none", steps=T_LONG, dt=DT)


def scene_batch(key):
    return KS.batch(**SCENES[key])


_REF = {}


def reference(O, key, persist=False):
    """The oracle's run of every scenario of a scene, every step recorded; computed once, shared with the GPU tests."""
    if (key, persist) not in _REF:
        out = []
        for sc in scene_batch(key):
            veh = (sc["kind"] == KS.KIND_AGENT_VEHICLE).any()
            out.append(O.rollout(sc["knot_off"], sc["knots"], sc["bbox"], sc["etype"], sc["kind"], 0, sc["t0"], sc["length"], sc["dt"],
                                 persist=persist, ctrl=KS.ctrl_rows(sc, O.DEFAULT_CTRL), max_steps=sc["steps"], record=True,
                                 actions=np.zeros((sc["steps"], 2)) if veh else None,  # (sg_rollout feeds such slots (0, 0))
                                 event_cap=EV_CAP, route_off=sc.get("route_off"), routes=sc.get("routes")))
        _REF[(key, persist)] = out
    return _REF[(key, persist)]


# ------------------------------------------------------------------------------------------------ the module itself
def test_clock_accumulates():
    c = KS.clock(0.37, 1 / 30, 50)
    t = 0.37
    for k in range(51):
        assert c[k] == t
        t += 1 / 30
    assert (KS.clock(0.0, 0.1, 40) != 0.1 * np.arange(41)).any()  # (not t0 + k * dt)


def test_scenes_are_deterministic_and_well_formed():
    for key in [("ragged", "E6"), ("clock", "E48"), ("twins", "E6_flat"), ("offset", "crowd"), ("long", "E64")]:
        kw = SCENES[key]
        for r in (0, kw["R"] - 1):
            a = scene_batch(key)[r]
            b = KS.scene(kw["family"], kw["E"], r, kw["ego"], kw["dt"], kw["steps"], kw.get("K", 10), kw.get("zpr", "half"), kw.get("crowd", False))
            assert all(np.array_equal(a[k], b[k]) for k in ("knots", "knot_off", "kind", "bbox"))
            off, kn = a["knot_off"], a["knots"]
            assert np.isfinite(kn).all()
            for e in range(kw["E"]):
                assert (np.diff(kn[off[e]:off[e + 1], 0]) > 0).all(), (key, r, e)  # strictly increasing times
    lifted = [bool((sc["knots"][:, [3, 5, 6]] != 0).any()) for sc in scene_batch(("ragged", "E6"))]
    assert lifted == [r % 2 == 1 for r in range(12)]
    assert not any((sc["knots"][:, [3, 5, 6]] != 0).any() for sc in scene_batch(("ragged", "E6_flat")))
    off = scene_batch(("offset", "E48"))[0]
    assert off["t0"] == KS.OFFSET_T0 and (off["knots"][:, 0] < 0).any()
    n = np.diff(scene_batch(("long", "E64"))[0]["knot_off"])
    assert ((n == 1) | ((n >= 128) & (n <= 256))).all() and (n > 1).sum() >= 56


# ------------------------------------------------------------------------------------------------ what the scenes reach
def _cov(key):
    return [KS.coverage(sc) for sc in scene_batch(key)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_clock_scenes_step_on_rows_and_bounds(shape):
    """clock: at least half of the steps land exactly on a union row; at least 10 (entity, step) pairs land on min_t and at
    least 10 on max_t (the inclusive presence bound)."""
    cov = _cov(("clock", shape))
    assert sum(c["on_row"] for c in cov) >= sum(c["steps"] for c in cov) / 2, cov
    assert sum(c["on_min"] for c in cov) >= 10 and sum(c["on_max"] for c in cov) >= 10, cov
    assert sum(c["come_and_go"] for c in cov) >= 3
    assert sum(c["below_first"] for c in cov) >= 1, cov  # (a step that ends on the double below the first union row)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ragged_scenes_have_several_rows_per_step(shape):
    cov = _cov(("ragged", shape))
    assert np.mean([c["rows_per_step"] for c in cov]) >= 3, cov
    if shape not in ("E6", "E6_flat", "E6_replay"):  # (six entities: some scenario may be all statics)
        assert min(c["rows_per_step"] for c in cov) >= 3, cov
    assert sum(c["on_row"] for c in _cov(("offset", shape))) == 0  # (a clock from 0.37: never on a row)


@pytest.mark.parametrize("shape", ["E64", "E64_replay", "E64_flat"])
def test_long_scenes_have_thousands_of_rows(shape):
    cov = _cov(("long", shape))
    assert min(c["rows"] for c in cov) > 8192, cov
    assert all(c["steps"] < 100 and c["rows_per_step"] > 100 for c in cov), cov


@pytest.mark.parametrize("shape", list(SHAPES))
def test_twin_scenes_have_rows_one_ulp_apart(shape):
    cov = _cov(("twins", shape))
    assert sum(c["ulp_pairs"] for c in cov) >= 50, cov
    assert sum(c["on_row"] for c in cov) >= 10  # (half the pool are clock values)
    within = 0
    for sc in scene_batch(("twins", shape)):  # ... and within an entity
        off, t = sc["knot_off"], sc["knots"][:, 0]
        within += sum(int((np.nextafter(t[off[e]:off[e + 1] - 1], np.inf) == t[off[e] + 1:off[e + 1]]).sum()) for e in range(len(off) - 1))
    assert within >= 20, within


# ------------------------------------------------------------------------------------------------ oracle == batch_reference
@pytest.mark.parametrize("key", list(SCENES), ids=["-".join(k) for k in SCENES])
def test_oracle_rollout_equals_batch_reference(oracle, key):
    """Replayed poses and presence of oracle.rollout(...)["poses"] against batch_reference at clock(...)[1:], bit for bit, on
    every scenario of the scene; every value the oracle returns is finite; the scene has a collision event."""
    kw = SCENES[key]
    ref = reference(oracle, key)
    events = 0
    for r, (sc, o) in enumerate(zip(scene_batch(key), ref)):
        assert o["n_steps"] == kw["steps"] and not o["is_done"], (key, r)
        c = KS.clock(sc["t0"], kw["dt"], kw["steps"])
        assert np.array_equal(o["t"], c), (key, r)
        slots, off, kn = KS.replayed(sc)
        want, present = KS.batch_reference(off, kn, c[1:])
        got = o["poses"][1:, slots]
        assert np.array_equal(~np.isnan(got[..., 0]), present), (key, r)
        assert np.isfinite(want).all()
        assert bits_equal(got, np.where(present[..., None], want, np.nan)), (key, r)
        seen = ~np.isnan(o["poses"][..., 0])
        assert np.isfinite(o["poses"][seen]).all() and np.isfinite(o["vels"][seen]).all() and np.isfinite(o["dists"]).all()
        assert np.isfinite([o["metric_ego_avg_speed"], o["metric_ego_max_speed"], o["metric_ego_distance_travelled"], o["final_t"]]).all()
        assert np.isfinite(o["extra"]).all()
        events += o["n_events"]
    assert events >= 1, key


@pytest.mark.parametrize("persist", [False, True])
@pytest.mark.parametrize("family", KS.FAMILIES)
def test_oracle_batch_eval_equals_batch_reference(oracle, family, persist):
    """sgo_batch_eval itself (all entities batched, ON the union rows, one ulp beside them and at the clock's times)."""
    key = (family, "E64") if family == "long" else (family, "E48")
    for sc in scene_batch(key)[:2]:
        ts = KS.union_grid(sc["knot_off"], sc["knots"])
        q = np.concatenate([KS.clock(sc["t0"], sc["dt"], sc["steps"]), ts, np.nextafter(ts, np.inf), np.nextafter(ts, -np.inf),
                            [ts[0] - 1.0, ts[-1] + 1.0]])
        want, wp = KS.batch_reference(sc["knot_off"], sc["knots"], q, persist)
        got, gp = oracle.batch_eval(sc["knot_off"], sc["knots"], q, persist)
        assert np.array_equal(gp, wp) and bits_equal(got, want)
        assert wp.all() if persist else not wp.all()


@pytest.mark.parametrize("family", KS.FAMILIES)
def test_batch_reference_equals_scipy(family):
    """batch_reference against the two interp1d calls of BatchReplayEntity.add_entities themselves."""
    pytest.importorskip("scipy.interpolate")
    key = (family, "E64") if family == "long" else (family, "E48")
    for sc in scene_batch(key)[:2]:
        ts = KS.union_grid(sc["knot_off"], sc["knots"])
        q = np.concatenate([KS.clock(sc["t0"], sc["dt"], sc["steps"]), ts[::7], np.nextafter(ts[::7], np.inf), [ts[0] - 1.0, ts[-1] + 1.0]])
        assert bits_equal(KS.batch_reference(sc["knot_off"], sc["knots"], q)[0], KS.scipy_reference(sc["knot_off"], sc["knots"], q))


# ------------------------------------------------------------------------------------------------ the pin from the real reference
GOLD_STEPS = 24
GOLD_RUNS = [(f, n, dt, r) for f in KS.FAMILIES for n, dt, r in (("dt10", 0.1, 0), ("dt30", 1 / 30, 1))]


@pytest.mark.parametrize("family,name,dt,r", GOLD_RUNS, ids=[f"{f}-{n}" for f, n, _, _ in GOLD_RUNS])
def test_oracle_reproduces_the_reference_on_knot_times(oracle, family, name, dt, r):
    """knots.npz (tests/golden/make_golden_knots.py): ScenarioGym rollouts of a small edition of every family -- replayed poses,
    presence, velocities, distances, collision rows, metrics and events bit for bit, persist off and on; the PID ego within
    CTRL_TOL -- and BatchReplayEntity.step itself at the clock's times."""
    from conftest import scenario_arrays
    from test_oracle_golden import CTRL_TOL, _check_run

    g = load_golden("knots")
    key = f"{family}/{name}"
    sc = scenario_arrays(g, key + "/scenario")
    E = len(sc["etype"])
    # the fixture's scenario is the generator's of today (the reference's constructor re-sums the headings, nothing else)
    mine = KS.scene(family, E, r, "replay", dt, GOLD_STEPS, K=24)
    assert np.array_equal(mine["knot_off"], sc["knot_off"]) and np.array_equal(mine["knots"][:, [0, 1, 2, 3, 5, 6]], sc["knots"][:, [0, 1, 2, 3, 5, 6]])
    assert np.abs(mine["knots"][:, 4] - sc["knots"][:, 4]).max() < 1e-12 and sc["t0"] == mine["t0"]
    kind = oracle.default_kinds(E, sc["ego"])
    _check_run(oracle, g, sc, key + "/replay_nopersist", True, kind=kind, dt=dt, max_steps=GOLD_STEPS)
    o = _check_run(oracle, g, sc, key + "/replay_persist", True, kind=kind, dt=dt, max_steps=GOLD_STEPS, persist=True)
    assert not np.isnan(o["poses"]).any()
    kind = kind.copy()
    kind[sc["ego"]] = oracle.KIND_AGENT_PID
    o = _check_run(oracle, g, sc, key + "/pid", False, kind=kind, dt=dt, max_steps=GOLD_STEPS)
    assert np.abs(o["extra"][:, sc["ego"]] - g[key + "/pid/extra"]).max() < CTRL_TOL
    others = np.arange(E) != sc["ego"]  # (everybody but the controlled ego: replayed, bit for bit)
    assert bits_equal(o["poses"][:, others], g[key + "/pid/poses"][:, others])
    q = KS.clock(sc["t0"], dt, GOLD_STEPS)
    for pname, persist in (("nopersist", False), ("persist", True)):
        poses, present = oracle.batch_eval(sc["knot_off"], sc["knots"], q, persist)
        ref = g[f"{key}/batch_{pname}"]
        assert np.array_equal(present, ~np.isnan(ref[:, :, 0]))
        assert bits_equal(np.where(present[..., None], poses, np.nan), ref)
        want, wp = KS.batch_reference(sc["knot_off"], sc["knots"], q, persist)
        assert np.array_equal(wp, present) and bits_equal(np.where(wp[..., None], want, np.nan), ref)


def test_the_pin_holds_ties():
    """The small editions do put the clock ON knots: steps on union rows in the clock and twins fixtures, entities entering or
    leaving on a step in the clock fixture, rows one ulp apart in the twins fixture, a thousand rows in the long one."""
    from conftest import scenario_arrays

    g = load_golden("knots")
    cov = {}
    for family, name, dt, r in GOLD_RUNS:
        sc = scenario_arrays(g, f"{family}/{name}/scenario")
        sc["kind"] = np.where(np.arange(len(sc["etype"])) == 0, KS.KIND_AGENT_REPLAY, KS.KIND_REPLAY)
        cov[(family, name)] = KS.coverage(sc, dt, GOLD_STEPS)
    assert all(cov[("clock", n)]["on_row"] >= GOLD_STEPS // 2 for n in ("dt10", "dt30")), cov
    assert sum(cov[("clock", n)]["on_min"] + cov[("clock", n)]["on_max"] for n in ("dt10", "dt30")) >= 2, cov
    assert all(cov[("twins", n)]["ulp_pairs"] >= 5 and cov[("twins", n)]["on_row"] >= 3 for n in ("dt10", "dt30")), cov
    assert all(cov[("long", n)]["rows"] > 600 for n in ("dt10", "dt30")), cov
    assert all(cov[("offset", n)]["on_row"] == 0 for n in ("dt10", "dt30")), cov


def test_fixture_regenerates_byte_for_byte(tmp_path):
    """make_golden_knots.py, run in a fresh interpreter with a random hash seed against the real reference, writes the committed
    knots.npz again, array by array and byte for byte (skipped where the reference is not installed)."""
    if not os.path.isdir("/root/reference/scenario_gym"):
        pytest.skip("the reference is not on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import regen_golden

    assert regen_golden.GENERATORS["make_golden_knots"] == ["knots"]
    regen_golden.run_generator("make_golden_knots", str(tmp_path))
    ok, n, bad = regen_golden.compare_file("knots", str(tmp_path))
    assert not bad and ok == n > 400, bad[:6]
    assert os.path.getsize(os.path.join(GOLDEN, "knots.npz")) < 1_000_000
