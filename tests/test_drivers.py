"""Per-entity vehicle actions: sg_set_drivers / sg_step_drivers (drive_kernel) and the Python layers over them.

1. twin run: the ego as SG_KIND_AGENT_VEHICLE under sg_step against the ego as the one driver under sg_step_drivers, bit for bit
2. several drivers per scenario against the oracle, fed to a second handle through sg_set_external_poses, bit for bit
   (and a CPU test that holds the scenes of driver_scenes.py to their purpose)
3. the real reference (tests/golden/drivers.npz): the oracle decomposition (CPU) and BatchedScenarioGym (GPU) at 1e-9, the bound
   test_batched_gym_with_external_actions_and_mixed_agents holds device poses to
4. lifecycle and refusals
5. VectorScenarioEnv(drivers=...), ScenarioGym with two policy agents
"""
import ctypes as C

import numpy as np
import pytest

import driver_scenes as DS
from conftest import load_golden, scenario_arrays

gpu = pytest.mark.gpu
R, STEPS, DT = DS.R, DS.STEPS, DS.DT
TERMS = ["max_length", "ego_collision"]


@pytest.fixture(scope="module")
def sga():
    import scenario_gym_amd as sga

    return sga


def _engine(sga, E, persist=False, n=R):
    return sga.RolloutEngine(n, E, timestep=DT, persist=persist, terminal_conditions=TERMS, event_capacity=16)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _snapshot(eng):
    """Everything a caller can read of a handle: every row of the state blocks, the whole sg_scenario_state, the metric rows, the
    events, the terminal flags."""
    from scenario_gym_amd.engine import SCEN_DTYPE

    st = eng.state(raw=True)
    rows, ev = eng.metrics()
    snap = {k: np.array(v) for k, v in st.items()}
    snap["scen"] = np.frombuffer(eng._d2h(eng._view.scen, eng.R, SCEN_DTYPE).tobytes(), np.uint8)
    for f in ("ego_avg_speed", "ego_max_speed", "ego_distance_travelled", "final_t", "n_steps", "done", "n_collisions"):
        snap["metric_" + f] = rows[f].copy()
    for f in ("t", "scenario", "other", "type"):
        snap["event_" + f] = ev[f].copy()
    snap["flags"] = eng.terminal_flags()
    return snap


def _assert_same(a, b, what, but_speed_of=None):
    """Bit for bit; but_speed_of = (scenario [n], slot [n]): the controller-speed cells of these slots are somebody else's business."""
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if k == "ctrl_state" and but_speed_of is not None:
            x, y = x.copy(), y.copy()
            x[but_speed_of[0], but_speed_of[1], 0] = 0.0
            y[but_speed_of[0], but_speed_of[1], 0] = 0.0
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), f"{what}: {k} differs"


# ---------------------------------------------------------------------------------------------------------------- 1. twin run
def _twin(E):
    """(scenes, ego slots, actions [STEPS, R, 2]): the ego of every scenario is its one driver.  Scenario 0: ego in slot 0; 1: in the
    last slot; 2: an ego whose trajectory starts a second after t0 (late spawn); 3: braking down to zero speed (allow_reverse 0);
    4: reversing (allow_reverse 1, no max_speed), ego in the middle; 5: max_speed set and reached.  Actions beyond max_steer /
    max_accel from step CALM on in every scenario."""
    egos = [0, E - 1, 2, 0, E // 2 if E // 2 != DS.VICTIM else 3, 0]
    roles = ["a", "a", "c", "a", "a", "a"]
    scs = DS.batch(E, [[(e, r)] for e, r in zip(egos, roles)], egos=egos, seed=11)
    acts = DS.actions(R, seed=5)
    scs[3]["ctrl"][egos[3], :4] = (0.5, 4.0, np.nan, 0.0)
    acts[:, 3, 0] = -9.0
    scs[4]["ctrl"][egos[4], :4] = (0.6, 5.0, np.nan, 1.0)
    acts[:, 4, 0] = -9.0
    scs[5]["ctrl"][egos[5], :4] = (0.4, 5.0, 6.5, 0.0)
    acts[:, 5, 0] = 9.0
    return scs, egos, acts


@gpu
@pytest.mark.parametrize("persist", [False, True])
@pytest.mark.parametrize("E", [5, 64, 65, 300, 520])
def test_twin_run_vehicle_ego_against_driver_ego(sga, E, persist):
    import torch

    scs, egos, acts = _twin(E)
    pb = DS.pack(scs)
    pa = DS.pack(scs)
    pa.kind[np.arange(R) * E + np.array(egos)] = DS.KIND_AGENT_VEHICLE
    A, B = _engine(sga, E, persist), _engine(sga, E, persist)
    A.upload(pa)
    B.upload(pb)
    B.set_drivers(np.arange(R), egos)
    _assert_same(_snapshot(A), _snapshot(B), "reset")
    speeds = []
    for k in range(STEPS):
        if k == 20:  # half of the scenarios start anew, the others go on
            mask = np.array([1, 0, 1, 0, 1, 0], np.uint8)
            A.reset_scenarios(mask)
            B.reset_scenarios(mask)
            _assert_same(_snapshot(A), _snapshot(B), "reset_scenarios")
        A.step(1, acts[k:k + 1])
        B.step_drivers(acts[k:k + 1], 1)
        a, b = _snapshot(A), _snapshot(B)
        _assert_same(a, b, f"step {k}")
        speeds.append(b["ctrl_state"][np.arange(R), egos, 0])
    speeds = np.array(speeds)
    # the variants happened: the late ego spawned, the braking ego stood still, the reversing one went backwards, the capped one was capped
    assert (speeds[:20, 3] == 0.0).any() and (speeds[:, 4] < 0.0).any() and (speeds[:, 5] == 6.5).any()
    # one call of 40 steps (device actions) against forty calls of one (host actions), and against sg_step's own 40-step call
    A.reset()
    B.reset()
    A.step(STEPS, acts)
    B.step_drivers(torch.as_tensor(acts, device="cuda:0").contiguous(), STEPS)
    one = _snapshot(B)
    _assert_same(_snapshot(A), one, "40 steps in one call")
    B.reset()
    for k in range(STEPS):
        B.step_drivers(acts[k:k + 1], 1)
    _assert_same(one, _snapshot(B), "one call against forty")
    A.close()
    B.close()


@gpu
def test_twin_late_ego_spawns(sga):
    """The late ego of the twin scenes is absent at the reset and in the scene at the end (so the NaN branch of the kernel ran)."""
    E = 5
    scs, egos, acts = _twin(E)
    B = _engine(sga, E)
    B.upload(DS.pack(scs))
    B.set_drivers(np.arange(R), egos)
    assert not B.state()["present"][2, egos[2]]
    B.step_drivers(acts, STEPS)
    st = B.state()
    assert st["present"][2, egos[2]] and st["ctrl_state"][2, egos[2], 0] != 0.0
    B.close()


@gpu
@pytest.mark.parametrize("policy", [False, True])
def test_one_step_routine_behind_three_entry_points(sga, policy):
    """Three twins of 2 scenarios x 4 entities with 2 drivers, 3 steps each: one call with host actions, one call with device actions,
    three sg_tick_drivers (no auto-reset, no progress term) with the same rows -- byte-identical raw state.  policy: the built-in
    policy runs the second driver, through sg_step_drivers_policy in the first two twins."""
    import torch

    E, n, steps = 4, 2, 3
    scs = DS.batch(E, [[(0, "a")], [(2, "free")]], seed=21)
    scen, slot = DS.driver_list(scs)
    acts = np.ascontiguousarray(DS.actions(n, seed=3)[:steps])
    d_acts = torch.as_tensor(acts, device="cuda:0").contiguous()
    before = d_acts.clone()
    twins = []
    for how in ("host", "device", "ticks"):
        eng = _engine(sga, E, n=2)
        eng.upload(DS.pack(scs))
        eng.set_drivers(scen, slot)
        if policy:
            sc = scs[1]
            eng.set_driver_policy([1], np.array([sga.idm_params(v0=5.0)]), [sc["knots"][sc["knot_off"][2]:sc["knot_off"][3], 1:3]])
        if how == "ticks":
            for k in range(steps):
                eng.tick_drivers(acts[k], auto_reset=False, w_progress=0.0)
        else:
            (eng.step_drivers_policy if policy else eng.step_drivers)(acts if how == "host" else d_acts, steps)
        eng.synchronize()
        twins.append(eng.state(raw=True))
        eng.close()
    assert torch.equal(d_acts, before)  # (the caller's device buffer is read, never written)
    assert (twins[0]["n_steps"] == steps).all()
    for how, st in zip(("device actions", "three ticks"), twins[1:]):
        for key in twins[0]:
            assert np.array_equal(_bits(twins[0][key]), _bits(st[key])), f"{how}: {key} differs"


# ------------------------------------------------------------------------------------------ 2. several drivers, against the oracle
CONFIGS ={"mixed65": (65, DS.mixed_config), "mixed520": (520, DS.mixed_config), "all65": (65, DS.all_config)}
_expected = {}


def _config(name, oracle):
    """(scenes, driver scenario [n], driver slot [n], actions [STEPS, n, 2], expected poses [STEPS + 1, n, 6], speeds [STEPS + 1, n]):
    computed once, shared by the tests, left unchanged."""
    if name not in _expected:
        E, cfg = CONFIGS[name]
        scs = DS.batch(E, cfg(E))
        scen, slot = DS.driver_list(scs)
        acts = DS.actions(len(scen))
        poses, speed, d0 = [], [], 0
        for sc in scs:
            nd = len(sc["drivers"])
            p, s = DS.expected_poses(oracle, sc, acts[:, d0:d0 + nd])
            poses.append(p)
            speed.append(s)
            d0 += nd
        _expected[name] = (scs, scen, slot, acts, np.concatenate(poses, axis=1), np.concatenate(speed, axis=1))
    return _expected[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_driver_scenes_do_what_they_are_for(oracle, name):
    """Every width: a step in which two drivers' boxes collide, a step in which a driver hits a replay entity (where there is one:
    not when every entity is a driver), a driver that spawns late, every driver more than 1 m from where its recorded trajectory
    ends.  Also: actions differ between drivers and from step to step, and go beyond the controllers' limits."""
    scs, scen, slot, acts, poses, speed = _config(name, oracle)
    E = CONFIGS[name][0]
    assert sorted({len(s["drivers"]) for s in scs}) == ([0, 1, 3] if name.startswith("mixed") else [E])
    assert {0, 63, 64} <= set(slot.tolist()) and (E != 520 or {255, 256, 519} <= set(slot.tolist()))
    assert len({acts[:, d].tobytes() for d in range(len(scen))}) == len(scen) and (np.diff(acts, axis=0) != 0).all()
    ctrl = np.array([scs[r]["ctrl"][s] for r, s in zip(scen, slot)])
    assert (np.abs(acts[..., 1]) > ctrl[:, 0]).any(axis=0).all() and (np.abs(acts[..., 0]) > ctrl[:, 1]).any(axis=0).all()
    dd = dr = late = 0
    for r, sc in enumerate(scs):
        mine = np.nonzero(scen == r)[0]
        if len(mine) == 0:
            continue
        kind = np.where(sc["kind"] == DS.KIND_AGENT_EXTERNAL, DS.KIND_REPLAY, sc["kind"]).astype(np.int32)
        o = oracle.rollout(sc["knot_off"], sc["knots"], sc["bbox"], sc["etype"], kind, sc["ego"], 0.0, sc["length"], DT, max_steps=STEPS,
                           force_steps=True)
        P = o["poses"].copy()
        P[:, slot[mine]] = poses[:, mine]
        late += int((np.isnan(poses[0, mine, 0]) & ~np.isnan(poses[-1, mine, 0])).any())
        for k in range(STEPS + 1):
            for s in slot[mine]:
                if np.isnan(P[k, s, 0]):
                    continue
                cs = oracle.corners(P[k, s], sc["bbox"][s])
                for e in np.nonzero(np.hypot(P[k, :, 0] - P[k, s, 0], P[k, :, 1] - P[k, s, 1]) < 8.0)[0]:
                    if e != s and oracle.quads_intersect(cs, oracle.corners(P[k, e], sc["bbox"][e])):
                        dd, dr = dd + int(e in slot[mine]), dr + int(e not in slot[mine])
        for d in mine:
            end = sc["knots"][sc["knot_off"][slot[d] + 1] - 1, 1:3]
            assert np.hypot(*(poses[-1, d, :2] - end)) > 1.0, (r, slot[d])
    assert dd > 0 and late > 0 and (dr > 0 or name == "all65")


@gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_several_drivers_against_the_oracle(sga, oracle, name):
    scs, scen, slot, acts, poses, speed = _config(name, oracle)
    E = CONFIGS[name][0]
    packed = DS.pack(scs)
    D, X = _engine(sga, E), _engine(sga, E)
    D.upload(packed)
    D.set_drivers(scen, slot)
    X.upload(packed)  # the same external slots, no driver list: their poses come from the oracle
    _assert_same(_snapshot(D), _snapshot(X), "reset", (scen, slot))
    assert np.array_equal(_bits(D.state()["ctrl_state"][scen, slot, 0]), _bits(speed[0]))
    for k in range(STEPS):
        fed = np.full((R, E, 6), np.nan)
        fed[scen, slot] = np.where(np.isnan(poses[k, :, :1]), np.nan, poses[k + 1])
        X.set_external_poses(fed)
        X.step(1)
        D.step_drivers(acts[k:k + 1], 1)
        d = _snapshot(D)
        _assert_same(d, _snapshot(X), f"step {k}", (scen, slot))
        assert np.array_equal(_bits(d["ctrl_state"][scen, slot, 0]), _bits(speed[k + 1])), f"step {k}: controller speeds"
    D.close()
    X.close()


# ----------------------------------------------------------------------------------------------------- 3. the real reference
def _golden_scene(g, i):
    a = scenario_arrays(g, f"{i}/scenario")
    E = len(a["etype"])
    drivers = [int(s) for s in g[f"{i}/drivers"]]
    kind = np.full(E, DS.KIND_REPLAY, np.int32)
    kind[a["ego"]] = DS.KIND_AGENT_REPLAY
    kind[drivers] = DS.KIND_AGENT_EXTERNAL
    ctrl = np.tile(DS.DEFAULT_CTRL, (E, 1))
    ctrl[drivers, :4] = g[f"{i}/ctrl"]
    return dict(a, kind=kind, ctrl=ctrl, drivers=drivers)


def test_oracle_decomposition_against_the_reference(oracle):
    """The expected-pose builder of test 2 on the reference's own run with three VehicleController agents in one scenario."""
    g = load_golden("drivers")
    assert int(g["steps"]) == STEPS and float(g["dt"]) == DT
    for i in range(int(g["n"])):
        sc = _golden_scene(g, i)
        poses, _ = DS.expected_poses(oracle, sc, g[f"{i}/actions"])
        want = g[f"{i}/poses"][:, sc["drivers"]]
        assert np.array_equal(np.isnan(poses), np.isnan(want)) and np.nanmax(np.abs(poses - want)) < 1e-9


def _preset_agent(sga):
    class PresetAgent(sga.Agent):
        """A Python policy over the built-in VehicleController: a preset (accel, steer) per tick."""

        def __init__(self, entity, actions, **kw):
            super().__init__(entity, sga.VehicleController(entity, **kw), sga.EgoLocalizationSensor(entity))
            self.actions, self.k = actions, 0

        def _reset(self):
            self.k = 0

        def _step(self, observation):
            a = self.actions[self.k]
            self.k += 1
            return sga.VehicleAction(a[0], a[1])

    return PresetAgent


def _golden_gym_setup(sga, g):
    from test_host_api import scenario_from_arrays

    PresetAgent = _preset_agent(sga)
    n = int(g["n"])
    scs = [scenario_from_arrays(scenario_arrays(g, f"{i}/scenario"), g[f"{i}/scenario/refs"]) for i in range(n)]
    where = {id(sc): i for i, sc in enumerate(scs)}

    def create_agent(s, e):
        i = where[id(s)]
        drivers = [int(k) for k in g[f"{i}/drivers"]]
        slot = s.entities.index(e)
        if slot in drivers:
            j = drivers.index(slot)
            c = g[f"{i}/ctrl"][j]
            return PresetAgent(e, g[f"{i}/actions"][:, j], max_steer=float(c[0]), max_accel=float(c[1]),
                               max_speed=None if np.isnan(c[2]) else float(c[2]), allow_reverse=bool(c[3]))
        if e.ref == "ego":
            return sga.ReplayTrajectoryAgent(e)

    return scs, create_agent


@gpu
def test_batched_gym_with_three_policy_agents_per_scenario(sga):
    """BatchedScenarioGym with three Python-policy agents over VehicleController in each of two scenarios -- the call that raised
    NotImplementedError before -- against the reference's poses, velocities and distances after every step."""
    g = load_golden("drivers")
    scs, create_agent = _golden_gym_setup(sga, g)
    gym = sga.BatchedScenarioGym(timestep=DT, terminal_conditions=[], record=True)  # (EgoLocalizationSensor reads recorded_poses)
    gym.set_scenarios(scs, create_agent=create_agent)
    assert len(gym._driver_agents) == 6 and not gym._policy_agents and gym.engine._n_drv == 6
    for k in range(STEPS + 1):
        for i, sc in enumerate(scs):
            st = gym.states[i]
            assert abs(st.t - g[f"{i}/t"][k]) < 1e-12
            for what, want in ((st.poses, g[f"{i}/poses"][k]), (st.velocities, g[f"{i}/vels"][k])):
                got = np.array([what.get(e, np.full(6, np.nan)) for e in sc.entities])
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.nanmax(np.abs(got - want)) < 1e-9, (k, i)
            got = np.array([st.distances[e] for e in sc.entities])
            assert np.max(np.abs(got - g[f"{i}/dists"][k])) < 1e-9, (k, i)
        if k < STEPS:
            gym.step()
    gym.close()


# --------------------------------------------------------------------------------------------------- 4. lifecycle and refusals
def _raw(eng):
    return eng.lib, eng.h


def _i32(x):
    return np.ascontiguousarray(x, np.int32)


@gpu
def test_lifecycle_and_refusals(sga):
    import scenario_gym_amd._lib as L

    E = 65
    cfg = [[(0, "a"), (63, "b"), (64, "c"), (5, "free")]] + [[(0, "a")]] * (R - 1)
    scs = DS.batch(E, cfg, seed=2)
    packed = DS.pack(scs)
    eng = _engine(sga, E)
    lib, h = _raw(eng)
    one_s, one_k = _i32([0]), _i32([0])
    assert lib.sg_set_drivers(h, 1, one_s.ctypes.data, one_k.ctypes.data) == -3  # SG_ERR_STATE before sg_upload
    assert lib.sg_step_drivers(h, 1, None, 0) == -3
    eng.upload(packed)
    assert lib.sg_step_drivers(h, 1, None, 0) == -3  # no list
    scen, slot = _i32([0, 0, 0, 1]), _i32([0, 63, 64, 0])  # (slot 5 of scenario 0: an external slot that is NOT a driver)
    eng.set_drivers(scen, slot)
    for bad_s, bad_k in (([R], [0]), ([-1], [0]), ([0], [E]), ([0], [-1]), ([0], [2]), ([0], [DS.VICTIM]), ([0, 1, 0], [0, 0, 0])):
        s, k = _i32(bad_s), _i32(bad_k)
        assert lib.sg_set_drivers(h, len(s), s.ctypes.data, k.ctypes.data) == -1, (bad_s, bad_k)
    assert lib.sg_set_drivers(h, -1, None, None) == -1 and lib.sg_set_drivers(h, 2, None, None) == -1
    assert lib.sg_step_drivers(h, 0, None, 0) == -1 and lib.sg_step_drivers(h, -3, None, 0) == -1
    # the refused calls left the list of four in place: NULL actions are zeros, and nothing beyond n_steps * n * 2 doubles is read
    other = _engine(sga, E)
    other.upload(packed)
    other.set_drivers(scen, slot)
    fed = np.full((R, E, 6), np.nan)
    fed[0, 5] = (3.0, -4.0, 0.0, 0.25, 0.0, 0.0)
    for e_ in (eng, other):
        e_.set_external_poses(fed)
    assert lib.sg_step_drivers(h, 3, None, 0) == 0
    buf = np.frombuffer(bytes([0xCC]) * (8 * (3 * 4 * 2 + 64)), np.float64).copy()
    buf[:3 * 4 * 2] = 0.0
    assert other.lib.sg_step_drivers(other.h, 3, buf.ctypes.data, 0) == 0
    a, b = _snapshot(eng), _snapshot(other)
    _assert_same(a, b, "NULL actions against zeros")
    assert np.isfinite(a["poses"][a["present"]]).all()
    # the external slot that is no driver went where sg_set_external_poses sent it, and stays there
    assert a["present"][0, 5] and np.array_equal(a["poses"][0, 5], fed[0, 5])
    # sg_rollout and sg_tick keep refusing such batches
    assert lib.sg_rollout(h, 4) == -3
    lay = _i32([0])
    d_obs, d_fl = C.c_void_p(), C.c_void_p()
    assert lib.sg_tick(h, None, 0, 20.0, 20.0, 8, 8, 1, lay.ctypes.data, C.byref(d_obs), C.byref(d_fl)) == -3
    # n == 0 clears the list; sg_upload forgets it
    eng.set_drivers([], [])
    assert lib.sg_step_drivers(h, 1, None, 0) == -3
    eng.set_drivers(scen, slot)
    assert lib.sg_step_drivers(h, 1, None, 0) == 0
    eng.upload(packed)
    assert lib.sg_step_drivers(h, 1, None, 0) == -3
    assert "sg_set_drivers" in L.SYMBOLS and "sg_step_drivers" in L.SYMBOLS
    eng.close()
    other.close()


# ------------------------------------------------------------------------------------------------------------ 5. Python layers
def _scenario_objects(scs):
    from test_host_api import scenario_from_arrays

    return [scenario_from_arrays(sc, ["ego" if i == sc["ego"] else f"entity_{i}" for i in range(len(sc["etype"]))]) for sc in scs]


@gpu
def test_vector_env_with_drivers(sga):
    """VectorScenarioEnv(drivers=...): shapes, equality with the engine calls, auto-reset restarting the drivers' speeds."""
    E = 8
    lists = [[0, 2, 3], [0], [], [3, 0], [2], [0, 2, 3]]
    roles = [["a", "b", "free"], ["a"], [], ["a", "b"], ["a"], ["a", "b", "free"]]
    scs = DS.batch(E, [list(zip(l, r)) for l, r in zip(lists, roles)], seed=4)
    for sc in scs[:2]:
        # two short episodes: they end (max_length) and start anew within the run
        for e in range(E):
            a, b = sc["knot_off"][e], sc["knot_off"][e + 1]
            if b - a == 2:
                sc["knots"][b - 1, 1:3] = sc["knots"][a, 1:3] + (sc["knots"][b - 1, 1:3] - sc["knots"][a, 1:3]) * (1.25 - sc["knots"][a, 0]) / (
                    sc["knots"][b - 1, 0] - sc["knots"][a, 0])
                sc["knots"][b - 1, 0] = 1.25
        sc["length"] = float(sc["knots"][:, 0].max())  # (Scenario.length: the last knot of any entity -- the static ones' 1.5)
    objs = _scenario_objects(scs)
    nd = sum(len(l) for l in lists)
    acts = DS.actions(nd, seed=9)
    env = sga.VectorScenarioEnv(objs, timestep=DT, n=8, terminal_conditions=["max_length"], max_steer=0.9, max_accel=5.0, drivers=lists)
    assert env.n_drivers == nd
    first = env.reset()
    assert first.shape == (nd, 2, 8, 8)
    # the same batch by hand
    packed = DS.pack(scs)
    scen, slot = DS.driver_list(scs)
    packed.ctrl[scen.astype(np.int64) * E + slot] = sga.ExternalVehicleAgent(objs[0].entities[0], max_steer=0.9, max_accel=5.0).controller.ctrl_row()
    eng = sga.RolloutEngine(R, E, timestep=DT, terminal_conditions=["max_length"])
    eng.upload(packed)
    eng.set_road_networks([], np.full(R, -1, np.int32))
    eng.set_drivers(scen, slot)
    eng.set_observers(scen, slot)
    restarted = np.zeros(R, bool)
    for k in range(20):
        obs, reward, done, info = env.step(acts[k])
        assert obs.shape == (nd, 2, 8, 8) and reward.shape == (R,) and done.shape == (R,)
        eng.step_drivers(acts[k:k + 1], 1)
        flags = eng.terminal_flags()
        want_done = (flags & 1) != 0
        assert np.array_equal(done, want_done) and np.array_equal(info["terminal_flags"], flags)
        assert np.array_equal(reward, np.where(want_done & ((flags & 12) != 0), -1.0, 0.01))
        if want_done.any():
            eng.reset_scenarios(want_done)
            restarted |= want_done
        assert np.array_equal(obs, eng.raster_map_observers([0, 1], 30.0, 30.0, 8, 8))
        a, b = env.engine.state(raw=True), eng.state(raw=True)
        for key in a:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), (k, key)
        if want_done.any():  # a restarted environment: its drivers' controller speeds are those of the reset, |velocity at t0|
            for d in np.nonzero(want_done[scen])[0]:
                v = a["vels"][scen[d], slot[d]]
                assert abs(a["ctrl_state"][scen[d], slot[d], 0] - np.hypot(v[0], v[1])) < 1e-12 and a["n_steps"][scen[d]] == 0
    assert restarted[:2].all() and not restarted[2:].any()
    env.close()
    eng.close()


@gpu
def test_vector_env_without_drivers_is_what_it_was(sga):
    """drivers=None: the ego as the handle's one external-action vehicle, one sg_tick per step -- the calls and the bytes of the
    environment before driver lists existed, over one episode."""
    from scenario_gym_amd.packing import pack_scenarios

    E = 8
    scs = DS.batch(E, [[]] * R, seed=6)
    objs = _scenario_objects(scs)
    env = sga.VectorScenarioEnv(objs, timestep=DT, n=8, terminal_conditions=["max_length"], auto_reset=False)
    assert env.n_drivers == 0 and (env.engine._n_drv, env.engine._n_obs) == (0, 0)
    packed, _ = pack_scenarios(objs, lambda s, e: sga.ExternalVehicleAgent(e, max_steer=0.9, max_accel=5.0) if e is s.ego else None)
    assert (packed.kind.reshape(R, E)[:, 0] == DS.KIND_AGENT_VEHICLE).all() and not (packed.kind == DS.KIND_AGENT_EXTERNAL).any()
    eng = sga.RolloutEngine(R, E, timestep=DT, terminal_conditions=["max_length"])
    eng.upload(packed)
    eng.set_road_networks([], np.full(R, -1, np.int32))
    acts = DS.actions(R, seed=12)
    assert np.array_equal(env.reset(), eng.raster_map([0, 1], 30.0, 30.0, 8, 8))
    for k in range(STEPS):
        obs, reward, done, info = env.step(acts[k])
        want, flags = eng.tick(acts[k], [0, 1], 30.0, 30.0, 8, 8)
        assert np.array_equal(obs, want) and np.array_equal(info["terminal_flags"], flags) and np.array_equal(done, (flags & 1) != 0)
        a, b = env.engine.state(raw=True), eng.state(raw=True)
        for key in a:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), (k, key)
        if done.any():
            break
    assert done.all() and k >= STEPS - 2
    env.close()
    eng.close()


@gpu
def test_scenario_gym_with_two_policy_agents(sga):
    """ScenarioGym (one scenario) with two Python-policy agents: the first two drivers of the golden's scene 0, the third entity
    replaying -- against the oracle decomposition, which test_oracle_decomposition_against_the_reference ties to the reference."""
    from oracle import oracle as O

    g = load_golden("drivers")
    scs, create_agent = _golden_gym_setup(sga, g)
    sc = _golden_scene(g, 0)
    third = sc["drivers"][2]

    def two(s, e):
        return None if s.entities.index(e) == third else create_agent(s, e)

    sc["kind"][third] = DS.KIND_REPLAY
    sc["drivers"] = sc["drivers"][:2]
    poses, _ = DS.expected_poses(O, sc, g["0/actions"][:, :2])
    gym = sga.ScenarioGym(timestep=DT, terminal_conditions=[])
    gym.set_scenario(scs[0], create_agent=two)
    for k in range(STEPS):
        gym.step()
        got = np.array([gym.state.poses.get(scs[0].entities[s], np.full(6, np.nan)) for s in sc["drivers"]])
        assert np.array_equal(np.isnan(got), np.isnan(poses[k + 1])) and np.nanmax(np.abs(got - poses[k + 1])) < 1e-9, k
    gym._b.close()
