"""The replay interpolant on per-entity knot times (tests/knot_scenes.py) in every rollout kernel family, through the C ABI.
Every comparison is exact: bits of every float, collision rows and events equal.

Every other device test uploads scenarios on one shared np.linspace grid: the union grid is that grid, stage 1 of
build_grid_kernel only reproduces knots, and the clock meets a grid row at t = 0 alone -- so the tie rule of
searchsorted(side="left"), the inclusive presence bound and the first-knot rule of the five restatements of the segment
cursor (sgym_core.hpp, sgym_wide.hpp, sgym_control.hpp, sgym_rollout.hpp, sgym_sensors.hpp, sgym_observers.hpp) decide
nothing there.  Here every scene is one tests/test_knot_times_cpu.py holds against the reference's two interp1d stages and
counts the ties of: steps ON union rows and one ulp beside them, entities entering and leaving ON a step, rows one ulp apart,
grids of more than 8,192 rows with a hundred rows per step, a clock that starts at 0.37.

CASES steers the dispatcher with the knobs of tests/test_gpu_variants.py and asserts sg_last_kernel().  A case compares the
recorded poses and the clock of every step, the final velocities, distances, controller state and collision rows, metric rows,
events and event classes (classify_events_kernel) of EVERY scenario with oracle.rollout.  The time-sliced kernels keep no
record: their cases compare the state after sg_rollout(k) for every k from 2 on.
"""
import numpy as np
import pytest

import box_scenes as B
import knot_scenes as KS
import test_gpu_variants as V
import test_knot_times_cpu as KC
from conftest import bits_equal
from test_gpu_variants import sga  # noqa: F401  (the fixture)

gpu = pytest.mark.gpu
EV_CAP = KC.EV_CAP
Q0, P0 = dict(SG_QUEUE="0"), dict(SG_PLANAR="0")

# (row, shape of test_knot_times_cpu.SHAPES, sg_last_kernel(), tuning, environment, slicing, persist)
ROWS = [
    ("plain-E6", "E6", "sg::rollout_kernel<8, 1, false, false>", V.NO_TAB, {}, False, False),
    ("plain-E48", "E48", "sg::rollout_kernel<64, 1, false, false>", V.NO_TAB, {}, False, False),
    ("plain-E48-persist", "E48", "sg::rollout_kernel<64, 1, false, false>", V.NO_TAB, {}, False, True),
    ("plain-E100", "E100", "sg::rollout_kernel<64, 2, false, false>", V.NO_TAB, {}, False, False),
    ("plain-E300", "E300", "sg::rollout_kernel<64, 8, false, false>", V.NO_TAB, {}, False, False),
    ("tab_rows-E48", "E48_replay", "sg::rollout_kernel<64, 1, false, true>", V.TAB, {}, False, False),
    ("tab_rows-E100", "E100", "sg::rollout_kernel<64, 2, false, true>", V.TAB, {}, False, False),
    ("tab-E6", "E6", "sg::rollout_kernel_tab<8>", V.TAB, dict(Q0, **P0), False, False),
    ("tab-E48-persist", "E48", "sg::rollout_kernel_tab<64>", V.TAB, dict(Q0, **P0), False, True),
    ("tab_planar-E6", "E6_flat", "sg::rollout_kernel_tab_planar<8>", V.TAB, Q0, False, False),
    ("tabq-E6", "E6", "sg::rollout_kernel_tabq<8>", V.TAB, P0, False, False),
    ("tabq_planar-E6", "E6_flat", "sg::rollout_kernel_tabq_planar<8>", V.TAB, {}, False, False),
    ("slice-E6", "E6_replay", "sg::rollout_kernel_slice<8>", {}, {}, "always", False),
    ("slice_tab-E6", "E6_flat", "sg::rollout_kernel_slice_tab<8>", {}, {}, "always", False),
    ("crowd_riders-E48", "crowd", "sg::rollout_kernel_crowd_riders<1>", V.TAB, {}, False, False),
    ("wide-E600", "wide", V.WIDE, V.NO_TAB, {}, False, False),
    ("wide-E600-persist", "wide", V.WIDE, V.NO_TAB, {}, False, True),
]
LONG_ROWS = [
    ("plain-E64", "E64", "sg::rollout_kernel<64, 1, false, false>", V.NO_TAB, {}, False, False),
    ("tab_rows-E64", "E64_replay", "sg::rollout_kernel<64, 1, false, true>", V.TAB, {}, False, False),
    ("tab-E64", "E64", "sg::rollout_kernel_tab<64>", V.TAB, dict(Q0, **P0), False, False),
    ("tabq_planar-E64", "E64_flat", "sg::rollout_kernel_tabq_planar<64>", V.TAB, {}, False, False),
    ("slice-E64", "E64_replay", "sg::rollout_kernel_slice<64>", {}, {}, "always", False),
]
CASES = [dict(id=f"{f}-{row[0]}", key=(f, row[1]), expect=row[2], tuning=row[3], env=row[4], slicing=row[5], persist=row[6])
         for f in KC.KNOT_FAMILIES for row in ROWS]
CASES += [dict(id=f"long-{row[0]}", key=("long", row[1]), expect=row[2], tuning=row[3], env=row[4], slicing=row[5], persist=row[6])
          for row in LONG_ROWS]


def test_cases_cover_the_scenes_and_the_families():
    """Every scene test_knot_times_cpu.py checks is uploaded by a case, every case uploads such a scene, and every family of
    knot times meets every kernel family of the list."""
    assert {c["key"] for c in CASES} == set(KC.SCENES)
    assert len({c["id"] for c in CASES}) == len(CASES)
    for f in KC.KNOT_FAMILIES:
        names = {c["expect"] for c in CASES if c["key"][0] == f}
        for part in ("<8, 1, false, false>", "<64, 1, false, false>", "<64, 2, false, false>", "<64, 8, false, false>", "false, true>",
                     "_tab<", "_tab_planar<", "_tabq<", "_tabq_planar<", "_slice<", "_slice_tab<", "crowd_riders<", "wide_move_kernel"):
            assert any(part in n for n in names), (f, part)
        assert {c["persist"] for c in CASES if c["key"][0] == f} == {False, True}


# ------------------------------------------------------------------------------------------------ helpers
def _pack(scs):
    from scenario_gym_amd.engine import DEFAULT_CTRL
    from scenario_gym_amd.packing import pack_arrays

    return pack_arrays(scs, kinds=[s["kind"] for s in scs], ctrls=[KS.ctrl_rows(s, DEFAULT_CTRL) for s in scs])


def _engine(sga, scs, case, record=True, **kw):
    steps = scs[0]["steps"]
    eng = sga.RolloutEngine(len(scs), len(scs[0]["kind"]), timestep=scs[0]["dt"], persist=case.get("persist", False),
                            record_capacity=steps + 1 if record else 0, event_capacity=EV_CAP, **kw)
    if case.get("tuning"):
        eng.set_tuning(**case["tuning"])
    eng.set_slicing(case.get("slicing", False))
    return eng


def _final(eng, packed, ref, where, rows_of=None):
    """Final state, metric rows, events and event classes of every scenario against the oracle results `ref`."""
    from oracle import check

    st = eng.state()
    rows, events = eng.metrics()
    E = packed.n_entities
    bad = {}
    for r, o in enumerate(ref):
        b = check.compare_final(st, rows, events, r, o, E, event_cap=EV_CAP, kind=packed.kind[r * E:(r + 1) * E])
        if b:
            bad[r] = b
    assert not bad, (where, bad)
    return st


def _recorded(eng, ref, steps, where):
    """The pose record: the clock and every entity's pose after the reset and after every step."""
    t, poses = eng.record(steps + 1)
    for r, o in enumerate(ref):
        assert np.array_equal(t[:, r], o["t"]), (where, "clock", r)
        E = o["poses"].shape[1]
        for k in range(steps + 1):
            assert bits_equal(poses[k, r, :E], o["poses"][k]), (where, "scenario", r, "pose after step", k,
                                                                np.nonzero((poses[k, r, :E] != o["poses"][k]).any(-1))[0][:8].tolist())


# ------------------------------------------------------------------------------------------------ every family, every kernel
@gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_knot_times_in_every_kernel_family(sga, oracle, monkeypatch, case):
    """One case of CASES: the dispatcher names the family; the record of every step, the final state, metric rows, events and
    event classes of every scenario equal the oracle's."""
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    scs = KC.scene_batch(case["key"])
    ref = KC.reference(oracle, case["key"], case["persist"])
    steps = scs[0]["steps"]
    packed = _pack(scs)
    eng = _engine(sga, scs, case, record=not case["slicing"])
    try:
        eng.upload(packed)
        if case["slicing"]:  # no record on this path: the state after sg_rollout(k), every k the path takes
            for k in range(2, steps):
                eng.rollout(k)
                assert eng.last_kernel() == case["expect"], (k, eng.last_kernel())
                st = eng.state()
                for r, o in enumerate(ref):
                    E = o["poses"].shape[1]
                    assert st["t"][r] == o["t"][k] and bits_equal(st["poses"][r, :E], o["poses"][k]), (case["id"], "rollout", k, "scenario", r)
                    assert bits_equal(st["vels"][r, :E], o["vels"][k]) and bits_equal(st["dists"][r, :E], o["dists"][k]), (case["id"], k, r)
        eng.rollout(steps)
        assert eng.last_kernel() == case["expect"], eng.last_kernel()
        if not case["slicing"]:
            _recorded(eng, ref, steps, case["id"])
        _final(eng, packed, ref, case["id"])
    finally:
        eng.close()
    assert sum(o["n_events"] for o in ref) > 0 and all(o["n_steps"] == steps for o in ref)


# ------------------------------------------------------------------------------------------------ the cursor from every side
CURSOR = [(f, "E48", "inline") for f in KC.KNOT_FAMILIES] + [(f, "E6_flat", "table") for f in KC.KNOT_FAMILIES] + \
         [("long", "E64", "inline"), ("long", "E64_flat", "table")]


@gpu
@pytest.mark.parametrize("family,shape,path", CURSOR, ids=["-".join(c) for c in CURSOR])
def test_cursor_from_every_side(sga, oracle, family, shape, path):
    """The cached segment cursor entered from every side, controllers inside the rollout kernel and through the pre-pass
    table: one sg_rollout(T); T calls of one step; 7 + (T - 7) steps; and a reset of every other scenario halfway, which rewinds
    its cursor -- each against the oracle, record and final state."""
    key = (family, shape)
    scs = KC.scene_batch(key)
    ref = KC.reference(oracle, key)
    steps, R = scs[0]["steps"], len(scs)
    half = steps // 2
    packed = _pack(scs)
    case = dict(tuning=V.NO_TAB if path == "inline" else V.TAB)
    eng = _engine(sga, scs, case)
    try:
        eng.upload(packed)
        eng.rollout(steps)
        assert ("tab" in eng.last_kernel()) == (path == "table"), eng.last_kernel()
        _recorded(eng, ref, steps, (key, "rollout"))
        _final(eng, packed, ref, (key, "rollout"))
        for name, calls in (("single steps", [1] * steps), ("7 + rest", [7, steps - 7])):
            eng.reset()
            for n in calls:
                eng.step(n)
            _recorded(eng, ref, steps, (key, name))
            _final(eng, packed, ref, (key, name))
        # half the steps, State.reset for the odd scenarios, half the steps again: the odd ones stand where a run of `half` steps ends
        mask = (np.arange(R) % 2).astype(np.uint8)
        short = [oracle.rollout(sc["knot_off"], sc["knots"], sc["bbox"], sc["etype"], sc["kind"], 0, sc["t0"], sc["length"], sc["dt"],
                                ctrl=KS.ctrl_rows(sc, oracle.DEFAULT_CTRL), max_steps=steps - half, record=True, event_cap=EV_CAP)
                 if mask[r] else ref[r] for r, sc in enumerate(scs)]
        eng.reset()
        eng.step(half)
        eng.reset_scenarios(mask)
        eng.step(steps - half)
        _final(eng, packed, short, (key, "masked reset"))
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("tuning", ["inline", "table"])
def test_one_handle_through_shared_and_ragged_grids(sga, oracle, tuning):
    """One handle, uploads in turn: a batch on ONE shared grid (a yard of box_scenes: the host's "one recording, one clock"
    shortcut), then ragged / clock / twins batches (its merge), the yard again, the offset batch -- every one equal to the oracle
    as on a fresh handle."""
    yard = B.batch("yard", 6, "sparse")
    yard_ref = [B.oracle_rollout(oracle, sc, B.steps_of(6), event_cap=EV_CAP) for sc in yard]
    for sc in yard:  # (what makes it the shortcut's case: every entity's knots lie on the scenario's one grid)
        assert len(np.unique(sc["knots"][:, 0])) == 6
    assert KC.T == B.steps_of(6) and KC.DT == B.DT and len(yard) == KC.SHAPES["E6"]["R"]
    eng = sga.RolloutEngine(len(yard), 6, timestep=B.DT, record_capacity=KC.T + 1, event_capacity=EV_CAP)
    try:
        eng.set_tuning(**(V.NO_TAB if tuning == "inline" else V.TAB))
        for stage in ("yard", "ragged", "clock", "yard", "twins", "offset", "yard"):
            if stage == "yard":
                from scenario_gym_amd.engine import DEFAULT_CTRL
                from scenario_gym_amd.packing import pack_arrays

                packed, ref = pack_arrays(yard, kinds=[s["kind"] for s in yard], ctrls=[B.ctrl_rows(s, DEFAULT_CTRL) for s in yard]), yard_ref
            else:
                packed, ref = _pack(KC.scene_batch((stage, "E6"))), KC.reference(oracle, (stage, "E6"))
            eng.upload(packed)
            eng.rollout(KC.T)
            _recorded(eng, ref, KC.T, (tuning, stage))
            _final(eng, packed, ref, (tuning, stage))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ observation consumers
@gpu
@pytest.mark.parametrize("family", ["clock", "twins"])
def test_observations_read_the_same_interpolant(sga, oracle, family):
    """The look-ahead detector (sg_future_collision_observers: every entity's recording sampled ahead of the clock) against
    oracle.future_collision, and the recorded-pose columns of the route observation (own_position_clamped at the clock) against
    test_routes.route_reference, for every entity of every scenario as an observer, at the reset -- t ON knots -- and after 9 and
    23 steps.  The horizons are multiples of the timestep: samples land on clock values, where these scenes have their knots."""
    from test_routes import route_reference, same

    key = (family, "E48")
    scs = KC.scene_batch(key)
    R, E = len(scs), 48
    scen, slot = np.repeat(np.arange(R), E), np.tile(np.arange(E), R)
    eng = _engine(sga, scs, dict(tuning=V.NO_TAB))
    hits = inside = outside = 0
    try:
        eng.upload(_pack(scs))
        eng.set_observers(scen, slot)
        for n_adv in (0, 9, 14):
            if n_adv:
                eng.step(n_adv)
            st = eng.state(raw=True)
            got = eng.route_observation(n_ahead=2, spacing=2.0, observers=True)
            want = route_reference(oracle, st, scs, scen, slot, {}, 2, 2.0)
            assert same(got, want), (family, n_adv, np.nonzero((np.asarray(got[0]) != want[0]).any(1) | (got[1] != want[1]).any(1))[0][:8].tolist())
            inside += int((want[1][:, 1] == 0).sum())
            outside += int((np.abs(want[1][:, 1]) == 1).sum())
            for horizon, n in ((1.0, 10), (0.3, 3), (0.37, 4)):
                flags = eng.future_collision_observers(horizon, n)
                ego = eng.future_collision(horizon, n)
                for j in range(R * E):
                    sc = scs[scen[j]]
                    w = oracle.future_collision(sc["knot_off"], sc["knots"], sc["bbox"], sc["kind"], slot[j], st["t"][scen[j]], horizon, n)
                    assert bool(flags[j]) == w, (family, n_adv, horizon, int(scen[j]), int(slot[j]))
                    assert slot[j] != 0 or bool(ego[scen[j]]) == w
                    hits += int(w)
    finally:
        eng.close()
    assert hits > 10 and inside > 100 and outside > 20, (hits, inside, outside)
