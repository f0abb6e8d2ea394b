"""The CPU oracle against golden vectors captured from the real reference (CPU-only tests).

Tolerances: replay poses / t / step counts / velocities / distances / metrics
bit-identical; controller-integrated poses <= 1e-5 abs (measured: < 1e-10); collisions exact.
"""
import os
import numpy as np
import pytest

from conftest import bits_equal, load_golden, scenario_arrays

CTRL_TOL = 1e-9  # measured worst 7.5e-11; the contract is 1e-5


# ---------------------------------------------------------------- T1/T2 trajectories
def test_position_at_t_modes(oracle):
    g = load_golden("trajectory")
    for i in range(int(g["pos/n"])):
        data, q = g[f"pos/{i}/data"], g[f"pos/{i}/q"]
        for name, (eb, ef) in dict(true=(1, 1), ff=(0, 0), ft=(0, 1), tf=(1, 0)).items():
            got = np.array([oracle.position_at_t(data, t, eb, ef) for t in q])
            assert bits_equal(got, g[f"pos/{i}/{name}"]), (i, name)
        none = g[f"pos/{i}/false_is_none"]
        for t, m, ref in zip(q, none, g[f"pos/{i}/false"]):
            got = oracle.position_at_t(data, t, 0, 0, none_outside=True)
            assert (got is None) == bool(m)
            if got is not None:
                assert bits_equal(got, ref)
        vel = np.array([oracle.velocity_at_t(data, t) for t in q])
        assert bits_equal(vel, g[f"pos/{i}/vel"]), i


def test_reference_known_answers_trajectory(oracle):
    """Inputs/expected values of the reference's own tests/test_trajectory.py:166-269, 112-128."""
    k = np.array([[0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0], [2, 2, 2, 0, 0, 0, 0]], np.float64)
    P = oracle.position_at_t
    assert np.allclose(P(k, 0.5, 1, 1)[:2], [0.5, 0.5])
    assert np.allclose(P(k, 1.5, 1, 1)[:2], [1.5, 1.5])
    assert np.allclose(P(k, 2.5, 1, 1)[:2], [2.5, 2.5])
    assert np.allclose(P(k, -1.0, 1, 1)[:2], [-1.0, -1.0])
    assert P(k, -1.0, 0, 0, none_outside=True) is None
    assert P(k, 3.0, 0, 0, none_outside=True) is None
    assert np.allclose(P(k, -1.0, 0, 1)[:2], [0.0, 0.0])
    assert np.allclose(P(k, 3.0, 1, 0)[:2], [2.0, 2.0])
    assert np.allclose(P(k, 3.0, 1, 1)[:2], [3.0, 3.0])
    one = np.array([[0.0, 1.0, 1.0, 0, 0, 0, 0]])
    assert np.allclose(P(one, 10.0, 0, 0)[:2], [1.0, 1.0])  # test_single_cp
    kv = np.array([[0, 0, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0], [2, 0, 2, 0, 0, 0, 0]], np.float64)
    V = oracle.velocity_at_t
    assert np.allclose(V(kv, 0.5)[:2], [0, 1])
    assert np.allclose(V(kv, 2.5)[:2], [0, 0])
    assert np.allclose(V(kv, 0.0)[:2], [0, 1])
    assert np.allclose(V(kv, 2.0)[:2], [0, 1])


# ---------------------------------------------------------------- B1/B2 batch replay
@pytest.mark.parametrize("key,persist", [("kat", False), ("rand0", False), ("rand1", True)])
def test_batch_replay(oracle, key, persist):
    g = load_golden("batch")
    poses, present = oracle.batch_eval(g[key + "/knot_off"], g[key + "/knots"], g[key + "/q"], persist)
    ref = g[key + "/poses"]
    assert np.array_equal(present, ~np.isnan(ref[:, :, 0]))
    poses[~present] = np.nan
    assert bits_equal(poses, ref)


def test_batch_known_answer(oracle):
    """tests/test_entity.py:40-77: static at origin, mover at (1.5, 0) at t=1, absent at t=5."""
    off = np.array([0, 1, 3])
    knots = np.array([[0.0, 0, 0, 0, 0, 0, 0], [0.0, 1, 0, 0, 0, 0, 0], [2.0, 2, 0, 0, 0, 0, 0]])
    poses, present = oracle.batch_eval(off, knots, [1.0, 5.0])
    assert np.allclose(poses[0, 0, :2], 0) and np.allclose(poses[0, 1, :2], [1.5, 0.0])
    assert present[1, 0] and not present[1, 1]


# ---------------------------------------------------------------- full rollouts
def _check_run(oracle, g, sc, p, exact, **kw):
    E = len(sc["etype"])
    o = oracle.rollout(**sc, **kw)
    assert o["n_steps"] == int(g[p + "/n_steps"]), p
    assert o["is_done"] == bool(g[p + "/is_done"])
    assert bits_equal(o["t"], g[p + "/t"]), p
    for k in ("poses", "vels", "dists"):
        if exact:
            assert bits_equal(o[k], g[p + "/" + k]), (p, k)
        else:
            assert np.array_equal(np.isnan(o[k]), np.isnan(g[p + "/" + k])), (p, k)
            assert np.nanmax(np.abs(o[k] - g[p + "/" + k])) < CTRL_TOL, (p, k)
    assert np.array_equal(oracle.coll_to_dense(o["coll"], E), g[p + "/coll"]), p
    for k in ("metric_ego_avg_speed", "metric_ego_max_speed", "metric_ego_distance_travelled"):
        if exact:
            assert o[k] == float(g[p + "/" + k]), (p, k)
        else:
            assert abs(o[k] - float(g[p + "/" + k])) < CTRL_TOL, (p, k)
    if p + "/ev_t" in g:
        assert np.array_equal(o["ev_t"], g[p + "/ev_t"]), p
        assert np.array_equal(o["ev_other"], g[p + "/ev_other"]), p
        assert all((t == 5) == (n == "non_vehicle") for t, n in zip(o["ev_type"], g[p + "/ev_type"]))
    return o


def test_xosc_scenarios_replay_bit_identical(oracle):
    g = load_golden("scenarios")
    for name in g["names"]:
        sc = scenario_arrays(g, f"{name}/scenario")
        kind = oracle.default_kinds(len(sc["etype"]), sc["ego"])
        for run, dt in (("dt30", 1 / 30), ("dt10", 0.1)):
            _check_run(oracle, g, sc, f"{name}/{run}", True, kind=kind, dt=dt)


def test_known_values_from_survey(oracle):
    """a5e43fe4: t0 = 5.087952, 377 steps, final t = 17.65461866666671;
    3fee6507 metrics inside the ranges asserted by tests/test_metrics.py:27-30."""
    g = load_golden("scenarios")
    sc = scenario_arrays(g, "a5e43fe4/scenario")
    o = oracle.rollout(**sc, kind=oracle.default_kinds(len(sc["etype"]), sc["ego"]), dt=1 / 30)
    assert sc["t0"] == 5.087952 and o["n_steps"] == 377 and o["final_t"] == 17.65461866666671
    sc = scenario_arrays(g, "3fee6507/scenario")
    o = oracle.rollout(**sc, kind=oracle.default_kinds(len(sc["etype"]), sc["ego"]), dt=1 / 30)
    assert 4 <= o["metric_ego_avg_speed"] <= 5
    assert 10 <= o["metric_ego_max_speed"] <= 12
    assert 90 <= o["metric_ego_distance_travelled"] <= 110
    assert o["n_events"] == 0


def test_vanishing_and_persist(oracle):
    """tests/test_scenario_gym.py:17-25, 68-97."""
    g = load_golden("scenarios")
    sc = scenario_arrays(g, "vanish/scenario")
    kind = oracle.default_kinds(len(sc["etype"]), sc["ego"])
    o = _check_run(oracle, g, sc, "vanish/nopersist", True, kind=kind, dt=0.1)
    assert np.isnan(o["poses"][-1, 1, 0])  # entity 1 absent at the end
    o = _check_run(oracle, g, sc, "vanish/persist", True, kind=kind, dt=0.1, persist=True)
    assert not np.isnan(o["poses"]).any()  # everyone present at every step


@pytest.mark.parametrize("i", range(4))
def test_synthetic_scenes(oracle, i):
    g = load_golden("synth")
    sc = scenario_arrays(g, f"{i}/scenario")
    E = len(sc["etype"])
    for dtn, dt in (("dt30", 1 / 30), ("dt10", 0.1)):
        kind = oracle.default_kinds(E, sc["ego"])
        _check_run(oracle, g, sc, f"{i}/replay_{dtn}_nopersist", True, kind=kind, dt=dt)
        _check_run(oracle, g, sc, f"{i}/replay_{dtn}_persist", True, kind=kind, dt=dt, persist=True)
        _check_run(oracle, g, sc, f"{i}/term_collision_{dtn}", True, kind=kind, dt=dt,
                   terminal_mask=oracle.TERM_MAX_LENGTH | oracle.TERM_COLLISION)
        _check_run(oracle, g, sc, f"{i}/term_ego_collision_{dtn}", True, kind=kind, dt=dt,
                   terminal_mask=oracle.TERM_MAX_LENGTH | oracle.TERM_EGO_COLLISION)
        kind = kind.copy()
        kind[sc["ego"]] = oracle.KIND_AGENT_PID
        o = _check_run(oracle, g, sc, f"{i}/pid_{dtn}", False, kind=kind, dt=dt)
        assert np.abs(o["extra"][:, sc["ego"]] - g[f"{i}/pid_{dtn}/extra"]).max() < CTRL_TOL
        kind[sc["ego"]] = oracle.KIND_AGENT_VEHICLE
        p = f"{i}/ext_{dtn}"
        o = _check_run(oracle, g, sc, p, False, kind=kind, dt=dt, actions=g[p + "/actions"],
                       max_steps=int(g[p + "/n_steps"]) + 3)
        assert np.abs(o["extra"][:, sc["ego"], 0] - g[p + "/extra"][:, 0]).max() < CTRL_TOL


def test_pid_agent_on_xosc(oracle):
    """tests/test_controller.py:7-25 configuration; 225 steps, final ego from SURVEY 8c G-F."""
    g = load_golden("pid_xosc")
    sc = scenario_arrays(g, "scenario")
    E = len(sc["etype"])
    kind = oracle.default_kinds(E, sc["ego"])
    kind[sc["ego"]] = oracle.KIND_AGENT_PID
    ctrl = np.tile(oracle.DEFAULT_CTRL, (E, 1))
    ctrl[:, 6], ctrl[:, 1], ctrl[:, 0] = g["params"]
    o = _check_run(oracle, g, sc, "run", False, kind=kind, dt=0.1, ctrl=ctrl)
    assert o["n_steps"] == 225
    assert np.allclose(o["poses"][-1, sc["ego"], [0, 1, 3]], [310.19444195, 368.25547349, 1.69257669], atol=1e-7)


# ---------------------------------------------------------------- G1/G2 geometry
def test_head_on_collision_event(oracle):
    """tests/test_utils.py:12-61 scene: no collision at start, collision at the end; at dt=0.1 the
    first (only) ego event is at t = 8.799999999999985 with entity_1, non_vehicle."""
    g = load_golden("collision")
    sc = scenario_arrays(g, "headon/scenario")
    o = _check_run(oracle, g, sc, "headon/run", True, kind=oracle.default_kinds(2, 0), dt=0.1)
    dense = oracle.coll_to_dense(o["coll"], 2)
    assert not dense[0].any() and dense[-1, 0, 1] and dense[-1, 1, 0]
    assert o["ev_t"].tolist() == [8.799999999999985] and o["ev_other"].tolist() == [1]
    assert o["ev_type"].tolist() == [5]


def test_corners_match_reference(oracle):
    g = load_golden("collision")
    got = np.array([oracle.corners(p, b) for p, b in zip(g["corners/poses"], g["corners/boxes"])])
    # np.cos/np.sin differ from the oracle's sincos in the last ulp -> 1e-12 abs at |xy| <= 200
    assert np.abs(got - g["corners/points"]).max() < 1e-12


def test_sincos_accuracy(oracle):
    """< 1 ulp against 60-digit mpmath, including arguments next to multiples of pi/2."""
    import mpmath as mp

    mp.mp.dps = 60
    rng = np.random.default_rng(1)
    xs = np.concatenate([
        rng.uniform(-8, 8, 400), rng.uniform(-3e4, 3e4, 400), rng.normal(0, 1e-3, 50),
        np.arange(-40, 41) * (np.pi / 2), np.nextafter(np.arange(1, 30) * (np.pi / 2), 0), [0.0, 0.3, 0.78125],
    ])
    worst = 0.0
    for x in xs:
        s, c = oracle.sincos(x)
        for got, ref in ((s, mp.sin(mp.mpf(float(x)))), (c, mp.cos(mp.mpf(float(x))))):
            ulp = np.spacing(abs(float(ref))) if float(ref) != 0 else 5e-324
            worst = max(worst, abs(float((mp.mpf(got) - ref) / ulp)))
    assert worst < 1.0, worst
    assert oracle.sincos(0.0) == (0.0, 1.0)


def test_pair_intersections_exact(oracle):
    """10^4 OBB pairs: (a) the fp64 SAT on the REFERENCE's corners equals the exact-rational label
    for every pair; (b) so does the SAT on the oracle's own corners (sincos differs by <= 1 ulp)."""
    g = load_golden("collision")
    lab = g["pairs/intersects"].astype(bool)
    got = np.array([oracle.quads_intersect(a, b) for a, b in zip(g["pairs/corners_a"], g["pairs/corners_b"])])
    assert np.array_equal(got, lab)
    own = np.array([
        oracle.quads_intersect(oracle.corners(pa, ba), oracle.corners(pb, bb))
        for pa, ba, pb, bb in zip(g["pairs/pose_a"], g["pairs/box_a"], g["pairs/pose_b"], g["pairs/box_b"])
    ])
    assert np.array_equal(own, lab)
    assert 0.2 < lab.mean() < 0.5


# ---------------------------------------------------------------- F1-F4 pedestrians / social force
def ped_inputs(g, si, oracle, max_speed=None):
    """Arrays for the closed-loop pedestrian goldens: kinds, controller rows, routes."""
    sc = scenario_arrays(g, f"loop{si}/scenario")
    E = len(sc["etype"])
    R, vdes = g[f"loop{si}/routes"], g[f"loop{si}/vdes"]
    thr = float(g[f"loop{si}/distance_threshold"]) if f"loop{si}/distance_threshold" in g else 1.0  # (agent.py:26: the default)
    kind = oracle.default_kinds(E, sc["ego"])
    ctrl = np.tile(oracle.DEFAULT_CTRL, (E, 1))
    roff, rows = [0], []
    for i in range(E):
        if not np.isnan(vdes[i]):
            kind[i] = oracle.KIND_AGENT_PEDESTRIAN
            ctrl[i, 9], ctrl[i, 12] = vdes[i], thr
            if max_speed is not None:
                ctrl[i, 10] = max_speed
            rows.append(R[i])
        roff.append(roff[-1] + (len(R[i]) if not np.isnan(vdes[i]) else 0))
    return sc, kind, ctrl, np.array(roff, np.int64), np.concatenate(rows)


PED_TOL = 1e-8  # measured worst 1.6e-10 (velocities); the contract for controller-integrated poses is 1e-5


@pytest.mark.parametrize("si", [0, 1])
def test_pedestrian_closed_loops(oracle, si):
    """PedestrianAgent + SocialForce + PedestrianController closed loops captured from the reference
    (12 / 20 pedestrians + a replayed vehicle, empty road network, noise off)."""
    g = load_golden("pedestrian")
    sc, kind, ctrl, roff, routes = ped_inputs(g, si, oracle)
    E = len(kind)
    for dtn, dt in (("dt30", 1 / 30), ("dt10", 0.1)):
        p = f"loop{si}/{dtn}"
        o = oracle.rollout(**sc, kind=kind, dt=dt, ctrl=ctrl, route_off=roff, routes=routes)
        assert o["n_steps"] == int(g[p + "/n_steps"]) and bits_equal(o["t"], g[p + "/t"])
        for k in ("poses", "vels", "dists"):
            assert np.array_equal(np.isnan(o[k]), np.isnan(g[p + "/" + k]))
            assert np.nanmax(np.abs(o[k] - g[p + "/" + k])) < PED_TOL, (p, k)
        ex = g[p + "/extra"]
        ped = ~np.isnan(ex[0, :, 0])
        assert np.array_equal(o["extra"][:, ped, 1], ex[:, ped, 1])              # goal_idx exact
        assert np.abs(o["extra"][:, ped] - ex[:, ped]).max() < PED_TOL           # speed, force
        assert np.array_equal(oracle.coll_to_dense(o["coll"], E), g[p + "/coll"])
        assert np.array_equal(o["ev_t"], g[p + "/ev_t"]) and np.array_equal(o["ev_other"], g[p + "/ev_other"])
        assert set(g[p + "/ev_type"]) <= {"non_vehicle"} and (o["ev_type"] == 5).all()


def test_social_force_math_accuracy(oracle):
    """exp / atan2 / tan shared with the kernels: < 2 ulp against 50-digit mpmath."""
    import mpmath as mp

    mp.mp.dps = 50
    rng = np.random.default_rng(3)

    def ulps(got, ref):
        return abs(float((mp.mpf(got) - ref) / np.spacing(abs(float(ref)))))

    w = max(ulps(oracle.exp(x), mp.e ** mp.mpf(float(x))) for x in rng.uniform(-30, 5, 1500))
    assert w < 1.0
    w = max(ulps(oracle.atan2(y, x), mp.atan2(mp.mpf(float(y)), mp.mpf(float(x)))) for y, x in rng.normal(0, 3, (1500, 2)))
    assert w < 2.0
    w = max(ulps(oracle.tan(x), mp.tan(mp.mpf(float(x)))) for x in rng.uniform(-1.4, 1.4, 1500))
    assert w < 2.0
    assert oracle.atan2(0.0, 0.0) == 0.0 and oracle.atan2(1.0, 0.0) == np.arctan2(1.0, 0.0) and oracle.exp(0.0) == 1.0


def test_radius_query_known_answers(oracle):
    """tests/test_state.py:74-101 style: strictly inside the 64-gon buffer, not the circle."""
    assert oracle.in_radius(0, 0, 10.0, 3.0, 4.0) and not oracle.in_radius(0, 0, 10.0, 30.0, 4.0)
    r = 10.0
    apothem = r * np.cos(np.pi / 64)
    mid = np.pi / 64  # direction of an edge midpoint
    assert oracle.in_radius(0, 0, r, (apothem - 1e-9) * np.cos(mid), -(apothem - 1e-9) * np.sin(mid))
    assert not oracle.in_radius(0, 0, r, (apothem + 1e-9) * np.cos(mid), -(apothem + 1e-9) * np.sin(mid))
    assert oracle.in_radius(0, 0, r, r - 1e-9, 0.0) and not oracle.in_radius(0, 0, r, r, 0.0)  # a vertex is not inside


def test_future_collision_detector_matches_reference(oracle):
    """FutureCollisionDetector (sensor/common.py:59-106) along the reference's own rollouts of five XOSC scenarios at two
    time steps and two horizons: the oracle's flag at every state time equals the reference's (2 x 3849 evaluations)."""
    from scenario_gym_amd.packing import default_kinds

    gs, g = load_golden("scenarios"), load_golden("sensors")
    n_pos = 0
    for name in g["names"]:
        s = scenario_arrays(gs, f"{name}/scenario")
        kind = default_kinds(len(s["bbox"]), int(s["ego"]))
        for dtn in ("dt30", "dt10"):
            ts, want = g[f"{name}/{dtn}/t"], g[f"{name}/{dtn}/future"]
            for hi, h in enumerate(g["horizons"]):
                got = np.array([oracle.future_collision(s["knot_off"], s["knots"], s["bbox"], kind, s["ego"], t, h) for t in ts])
                assert np.array_equal(got, want[:, hi].astype(bool)), (name, dtn, h)
                n_pos += int(got.sum())
    assert n_pos > 300


def test_raster_entity_layer_matches_reference(oracle):
    """RasterizedMapSensor "entity" layer (sensor/map.py:120-192) on every 4th state of the reference's dt = 0.1 rollouts
    of five XOSC scenarios, 30 x 30 over 30 m and 24 x 24 over 12 m: every cell equals the reference's."""
    gs, g = load_golden("scenarios"), load_golden("sensors")
    cells = ones = 0
    for name in g["names"]:
        s = scenario_arrays(gs, f"{name}/scenario")
        poses = gs[f"{name}/dt10/poses"]
        for k, (w, h, n) in enumerate(g["raster_cfg"]):
            want = g[f"{name}/dt10/map{k}"].astype(bool)
            for f, step in enumerate(g[f"{name}/dt10/map_steps"]):
                got = oracle.raster_entities(poses[step], s["bbox"], s["ego"], w, h, int(n), int(n))
                assert np.array_equal(got, want[f]), (name, k, step, int((got != want[f]).sum()))
                cells += got.size
                ones += int(got.sum())
    assert cells > 300000 and ones > 10000


def test_all_reference_scenarios_roll_out(oracle):
    """tests/test_scenarios.py of the reference rolls out every shipped OpenSCENARIO file: the oracle reproduces the real
    reference on all 23 -- clock of every step, poses of every 25th step and of the last, final velocities, distances,
    collision adjacency and the three ego metrics, bit for bit."""
    from scenario_gym_amd.packing import default_kinds

    g = load_golden("all_scenarios")
    assert len(g["names"]) == 23
    for name in g["names"]:
        s = scenario_arrays(g, f"{name}/scenario")
        E = len(s["bbox"])
        o = oracle.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], default_kinds(E, s["ego"]), s["ego"], s["t0"],
                           s["length"], 1 / 30)
        assert bits_equal(o["t"], g[f"{name}/t"]), name
        assert bits_equal(o["poses"][::25][: len(g[f"{name}/keyframes"])], g[f"{name}/keyframes"]), name
        assert bits_equal(o["poses"][-1], g[f"{name}/final_poses"]) and bits_equal(o["vels"][-1], g[f"{name}/final_vels"]), name
        assert bits_equal(o["dists"][-1], g[f"{name}/final_dists"]), name
        assert np.array_equal(oracle.coll_to_dense(o["coll"], E)[-1], g[f"{name}/final_coll"]), name
        for k in ("ego_avg_speed", "ego_max_speed", "ego_distance_travelled"):
            assert o["metric_" + k] == float(g[f"{name}/metric_{k}"]), (name, k)


# ---------------------------------------------------------------- road surfaces (N2 map layers, N4 ego_off_road)
ROAD_BITS = dict(driveable_surface=1, road=2, intersection=4, lane=8, walkable_surface=16, pavement=32, crossing=64)


def road_arrays(g, net):
    return {k: g[f"net/{net}/{k}"] for k in ("ring_off", "vert_off", "verts", "layers")}


def test_surface_contains_known_answers(oracle):
    """Every union the reference takes of its road-network polygons (driveable / walkable surface, the map layers), on the
    six shipped networks: 2,300 points each -- random, ON polygon vertices, a nanometre beside them, on edge midpoints --
    answered exactly as the exact-rational crossing number of the golden generator."""
    g = load_golden("roads")
    for net in g["networks"]:
        arr = oracle.RoadNetworkArrays(road_arrays(g, net))
        pts = g[f"net/{net}/points"]
        for name, bit in ROAD_BITS.items():
            got = oracle.surface_contains(arr, bit, pts[:, 0], pts[:, 1])
            assert np.array_equal(got, g[f"net/{net}/contains_{name}"].astype(bool)), (net, name)
    assert not oracle.surface_contains(None, 1, [0.0], [0.0])[0]  # no road network: every surface is empty


def test_orientation_sign_is_exact(oracle):
    """Points a few ulps off long edges: the fp64 determinant is noise there, the expansion sum decides."""
    from fractions import Fraction as F

    rng = np.random.default_rng(3)
    for _ in range(300):
        a, b = rng.uniform(-1000, 1000, 2), rng.uniform(-1000, 1000, 2)
        c = a + (b - a) * rng.uniform(0.1, 0.9)  # (nearly) on the edge a-b of the triangle a, b, far
        c = np.nextafter(c, c + rng.choice([-1, 1], 2) * rng.integers(0, 3, 2))
        far = a + np.array([-(b - a)[1], (b - a)[0]])  # to the left of a->b
        tri = dict(ring_off=[0, 1], vert_off=[0, 3], verts=[a, b, far], layers=[1])
        det = (F(a[0]) - F(c[0])) * (F(b[1]) - F(c[1])) - (F(a[1]) - F(c[1])) * (F(b[0]) - F(c[0]))
        # strictly left of a->b (and far from the other two edges) <=> strictly inside
        assert oracle.surface_contains(tri, 1, [c[0]], [c[1]])[0] == (det > 0)


def test_raster_map_layers_match_reference(oracle):
    """RasterizedMapSensor with all eight layers (sensor/map.py:136-271; the case of tests/test_sensor.py:38-77 and the
    default 20 x 20 grid) along the reference's rollouts of one scenario per shipped road network."""
    from scenario_gym_amd.packing import default_kinds

    g = load_golden("roads")
    layers = [0] + [ROAD_BITS[str(x)] for x in g["layers"][1:]]
    for n in g["scenarios"]:
        s = scenario_arrays(g, f"{n}/scenario")
        E = len(s["bbox"])
        o = oracle.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], default_kinds(E, s["ego"]), s["ego"], s["t0"],
                           s["length"], 0.1)
        net = oracle.RoadNetworkArrays(road_arrays(g, str(g[f"{n}/network"])))
        for c, (w, h, k) in enumerate(g["raster_cfg"]):
            want = g[f"{n}/map{c}"].astype(bool)
            for f, step in enumerate(g[f"{n}/map_steps"]):
                got = oracle.raster_map(o["poses"][step], s["bbox"], 0, net, layers, width=w, height=h, nw=int(k), nh=int(k))
                assert np.array_equal(got, want[f]), (n, c, step)
        assert want[:, 1].any() and want[0, 0, int(k) // 2, int(k) // 2]  # tests/test_sensor.py:55-61


def test_ego_off_road_terminal_matches_reference(oracle):
    """terminal_conditions=["max_length", "ego_off_road"] (state/state.py:397-407): the recorded egos stay on the road to
    the end; copies drifting sideways stop at the reference's step."""
    from scenario_gym_amd.packing import default_kinds

    g = load_golden("roads")
    stopped_early = 0
    for n in g["scenarios"]:
        net = oracle.RoadNetworkArrays(road_arrays(g, str(g[f"{n}/network"])))
        for tag in ("onroad", "drift"):
            s = scenario_arrays(g, f"{n}/{tag}/scenario")
            E = len(s["bbox"])
            o = oracle.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], default_kinds(E, s["ego"]), s["ego"],
                               s["t0"], s["length"], 0.1, terminal_mask=oracle.TERM_MAX_LENGTH | oracle.TERM_EGO_OFF_ROAD,
                               road=net)
            assert bits_equal(o["t"], g[f"{n}/{tag}/t"]), (n, tag)
            assert bits_equal(o["poses"][-1, s["ego"]], g[f"{n}/{tag}/final_ego"]), (n, tag)
            stopped_early += o["t"][-1] + 0.2 < s["length"]
        # without a road network the driveable surface is empty: off the road at once
        o = oracle.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], default_kinds(E, s["ego"]), s["ego"], s["t0"],
                           s["length"], 0.1, terminal_mask=oracle.TERM_EGO_OFF_ROAD)
        assert o["n_steps"] == 1
    assert stopped_early >= 2


@pytest.mark.parametrize("si", [0, 1])
def test_pedestrians_beside_a_building(oracle, si):
    """The boundary terms of the social force (pedestrian/social_force.py:86-104, 190-211) on the road network of
    examples/crowds.py (road, pavements, one building): a crowd walking along the pavement beside the building wall, some
    starting inside the building.  The repulsion from the wall reaches 19 (U / R = 20); reference closed loops at two time
    steps.  Without the road network the same crowd walks elsewhere."""
    g = load_golden("ped_roads")
    sc, kind, ctrl, roff, routes = ped_inputs(g, si, oracle)
    E = len(kind)
    net = oracle.RoadNetworkArrays({k: g[f"net/{k}"] for k in ("ring_off", "vert_off", "verts", "layers")})
    for dtn, dt in (("dt30", 1 / 30), ("dt10", 0.1)):
        p = f"loop{si}/{dtn}"
        o = oracle.rollout(**sc, kind=kind, dt=dt, ctrl=ctrl, route_off=roff, routes=routes, road=net)
        assert o["n_steps"] == int(g[p + "/n_steps"]) and bits_equal(o["t"], g[p + "/t"])
        for k in ("poses", "vels", "dists"):
            assert np.array_equal(np.isnan(o[k]), np.isnan(g[p + "/" + k]))
            assert np.nanmax(np.abs(o[k] - g[p + "/" + k])) < PED_TOL, (p, k)
        ex = g[p + "/extra"]
        ped = ~np.isnan(ex[0, :, 0])
        assert np.array_equal(o["extra"][:, ped, 1], ex[:, ped, 1])
        assert np.abs(o["extra"][:, ped] - ex[:, ped]).max() < PED_TOL
        assert np.abs(ex[:, ped, 2:]).max() > 15  # the wall is felt
        assert np.array_equal(oracle.coll_to_dense(o["coll"], E), g[p + "/coll"])
        free = oracle.rollout(**sc, kind=kind, dt=dt, ctrl=ctrl, route_off=roff, routes=routes)
        assert np.nanmax(np.abs(free["poses"] - g[p + "/poses"][: len(free["poses"])])) > 0.1


def test_collision_types_match_reference_code(oracle):
    """CollisionMetric.record_collision / get_collision_point / angle_between (metrics/collision.py:13-22, 81-203) run by
    the golden generator on 47 scenes with `Entity.pose` read as state.poses[entity] (the attribute is missing at this
    commit, see make_golden_collision_types.py): every event's time, hazard and type (t_bone, head_on, rear_end,
    side_swipe, non_vehicle) equals the reference's."""
    from scenario_gym_amd.packing import default_kinds

    g = load_golden("collision_types")
    seen = set()
    for n in g["names"]:
        s = scenario_arrays(g, f"{n}/scenario")
        E = len(s["bbox"])
        o = oracle.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], default_kinds(E, s["ego"]), s["ego"], s["t0"],
                           s["length"], 0.05, record=False)
        assert np.array_equal(o["ev_t"], g[f"{n}/ev_t"]) and np.array_equal(o["ev_other"], g[f"{n}/ev_other"]), n
        assert np.array_equal(o["ev_type"], g[f"{n}/ev_type"]), (n, o["ev_type"], g[f"{n}/ev_type"])
        # CollisionPointMetric (:242-253): intersection centroid and relative heading (box corners differ from numpy's by
        # <= 1 ulp of sin / cos)
        assert o["ev_point"].shape == g[f"{n}/ev_point"].shape
        assert len(o["ev_point"]) == 0 or np.abs(o["ev_point"] - g[f"{n}/ev_point"]).max() < 1e-10, n
        seen |= set(o["ev_type"].tolist())
    assert seen == {1, 2, 3, 4, 5}


def test_rss_distances_and_metric_match_reference(oracle):
    """RSSDistances + RSS (metrics/rss/callback.py, rss.py; tests/test_rss.py:5-25) on the reference's shipped scenarios
    and on synthetic traffic around the ego: every record the callback appended to its per-entity history (safe / lateral /
    longitudinal / both / unsafe_lateral / unsafe_longitudinal / found), the safe distances it computed, and the two
    metric flags."""
    from scenario_gym_amd.packing import default_kinds

    g = load_golden("rss")
    n_unsafe = 0
    for n in g["names"]:
        s = scenario_arrays(g, f"{n}/scenario")
        E = len(s["bbox"])
        o = oracle.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], default_kinds(E, s["ego"]), s["ego"], s["t0"],
                           s["length"], 0.1)
        assert bits_equal(o["t"], g[f"{n}/t"]), n
        r = oracle.rss_rollout(o, s["bbox"], s["ego"])
        want_code, want_safe = g[f"{n}/code"], g[f"{n}/safe"]
        assert np.array_equal(r["code"], want_code), (n, np.argwhere(r["code"] != want_code)[:5])
        upd = want_code >= 0
        assert np.abs(r["safe"][upd] - want_safe[upd]).max() < 1e-9, n
        assert r["safe_longitudinal"] == bool(g[f"{n}/safe_longitudinal"]) and r["safe_lateral"] == bool(g[f"{n}/safe_lateral"]), n
        n_unsafe += (want_code == 4).sum() + (want_code == 5).sum()
    assert n_unsafe > 30


@pytest.mark.parametrize("si", [0, 1, 2])
def test_pedestrian_noise_closed_loops(oracle, si):
    """The random fluctuations of SocialForce._step (pedestrian/social_force.py:106-114): closed loops of the reference
    with std_lon / std_lat > 0 after np.random.seed(k) (the third one with the reference's DEFAULT std).  The oracle
    consumes the same legacy stream -- np.random.RandomState(k).standard_normal -- two variates per walking pedestrian per
    step in agent order, and lands on the reference's trajectories; it consumes exactly as many variates as numpy did."""
    g = load_golden("ped_noise")
    sc, kind, ctrl, roff, routes = ped_inputs(g, si, oracle)
    E = len(kind)
    std_lon, std_lat, seed = g[f"loop{si}/noise"]
    used = int(g[f"loop{si}/variates_used"])
    normals = np.random.RandomState(int(seed)).standard_normal(used + 64)
    p = f"loop{si}/dt30"
    o = oracle.rollout(**sc, kind=kind, dt=1 / 30, ctrl=ctrl, route_off=roff, routes=routes,
                       noise=dict(mode="stream", std_lon=std_lon, std_lat=std_lat, normals=normals))
    assert o["n_steps"] == int(g[p + "/n_steps"]) and bits_equal(o["t"], g[p + "/t"])
    assert o["noise_used"] == used
    for k in ("poses", "vels", "dists"):
        assert np.array_equal(np.isnan(o[k]), np.isnan(g[p + "/" + k]))
        assert np.nanmax(np.abs(o[k] - g[p + "/" + k])) < PED_TOL, (p, k)
    ex = g[p + "/extra"]
    ped = ~np.isnan(ex[0, :, 0])
    assert np.array_equal(o["extra"][:, ped, 1], ex[:, ped, 1])              # goal_idx exact
    assert np.abs(o["extra"][:, ped] - ex[:, ped]).max() < PED_TOL           # speed, force
    assert np.array_equal(oracle.coll_to_dense(o["coll"], E), g[p + "/coll"])
    assert np.array_equal(o["ev_t"], g[p + "/ev_t"]) and np.array_equal(o["ev_other"], g[p + "/ev_other"])
    # without the noise the trajectories differ (the test would pass trivially otherwise)
    o0 = oracle.rollout(**sc, kind=kind, dt=1 / 30, ctrl=ctrl, route_off=roff, routes=routes)
    assert np.nanmax(np.abs(o0["poses"][: o["n_steps"] + 1] - o["poses"])) > (1e-3 if si < 2 else 1e-9)


@pytest.mark.parametrize("si", [0, 1, 2, 3])
def test_random_walk_closed_loops(oracle, si):
    """RandomWalk (pedestrian/random_walk.py:22-44) closed loops of the reference after np.random.seed(k): speed =
    np.random.normal(speed_desired + bias_lon, std_lon), heading = np.random.normal(angle to the goal point + bias_lat,
    std_lat) -- with a bias and a max_speed that clips (loop 1), the reference's default parameters (loop 2) and std 0
    (loop 3: the variates are still drawn).  The oracle consumes the same legacy stream and lands on the reference's
    trajectories, speeds, goal indices and (zero) forces, with exactly as many variates as numpy handed out."""
    g = load_golden("random_walk")
    std_lon, std_lat, bias_lon, bias_lat, max_speed, seed = g[f"loop{si}/params"]
    sc, kind, ctrl, roff, routes = ped_inputs(g, si, oracle, max_speed=max_speed)
    E = len(kind)
    used = int(g[f"loop{si}/variates_used"])
    normals = np.random.RandomState(int(seed)).standard_normal(used + 64)
    sf = oracle.social_force_params(bias_lon=bias_lon, bias_lat=bias_lat)
    p = f"loop{si}/dt30"
    o = oracle.rollout(**sc, kind=kind, dt=1 / 30, ctrl=ctrl, route_off=roff, routes=routes, sf=sf, behaviour="random_walk",
                       noise=dict(mode="stream", std_lon=std_lon, std_lat=std_lat, normals=normals))
    assert o["n_steps"] == int(g[p + "/n_steps"]) and bits_equal(o["t"], g[p + "/t"])
    assert o["noise_used"] == used
    for k in ("poses", "vels", "dists"):
        assert np.array_equal(np.isnan(o[k]), np.isnan(g[p + "/" + k]))
        assert np.nanmax(np.abs(o[k] - g[p + "/" + k])) < PED_TOL, (p, k)
    ex = g[p + "/extra"]
    ped = ~np.isnan(ex[0, :, 0])
    assert np.array_equal(o["extra"][:, ped, 1], ex[:, ped, 1])              # goal_idx exact
    assert np.abs(o["extra"][:, ped] - ex[:, ped]).max() < PED_TOL           # controller speed; force
    assert not ex[:, ped, 2:].any() and not o["extra"][:, ped, 2:].any()     # RandomWalk never touches agent.force
    assert np.array_equal(oracle.coll_to_dense(o["coll"], E), g[p + "/coll"])
    assert np.array_equal(o["ev_t"], g[p + "/ev_t"]) and np.array_equal(o["ev_other"], g[p + "/ev_other"])
    if si == 1:
        assert (np.abs(ex[1:, ped, 0]) == max_speed).any()                   # the controller's clip did act
    # the social force model on the same inputs walks elsewhere (the test would pass trivially otherwise)
    o0 = oracle.rollout(**sc, kind=kind, dt=1 / 30, ctrl=ctrl, route_off=roff, routes=routes, sf=sf,
                        noise=dict(mode="stream", std_lon=std_lon, std_lat=std_lat, normals=normals))
    n = min(o0["n_steps"], o["n_steps"]) + 1
    assert np.nanmax(np.abs(o0["poses"][:n] - o["poses"][:n])) > 1e-3


def mixed_model_rows(g, si, oracle):
    """mixed_peds.npz loop si: the oracle's model rows (oracle.ped_model_row) and the model of every entity (0 where none)."""
    cols = [str(c) for c in g["model_cols"]]
    rows = []
    for row in g[f"loop{si}/models"]:
        m = dict(zip(cols, row))
        sf = oracle.social_force_params(m["relaxation_time"] or 1.5, m["ped_repulse_V"], m["ped_repulse_sigma"] or 1.0, m["ped_attract_C"],
                                        m["sight_weight"], bool(m["sight_weight_use"]), m["sight_angle"], m["max_speed_factor"],
                                        m["bias_lon"], m["bias_lat"])
        rows.append(oracle.ped_model_row("random_walk" if m["behaviour"] == 1 else "social_force", sf, m["std_lon"], m["std_lat"]))
    return np.array(rows), np.maximum(g[f"loop{si}/model_of"], 0).astype(np.int32)


@pytest.mark.parametrize("si", [0, 1, 2, 3])
def test_mixed_pedestrian_models_closed_loops(oracle, si):
    """Every PedestrianAgent of the reference holds its OWN behaviour object (pedestrian/agent.py:18-41): closed loops with
    SocialForce pedestrians of two or three parameter sets and RandomWalk pedestrians in one scenario, after
    np.random.seed(k) (mixed_peds.npz, make_golden_mixed_peds.py).  The oracle steps every pedestrian under its own model,
    draws the two variates per walking pedestrian in agent order from the same legacy stream, and lands on the reference's
    trajectories, speeds, goal indices and forces with exactly as many variates as numpy handed out."""
    g = load_golden("mixed_peds")
    sc, kind, ctrl, roff, routes = ped_inputs(g, si, oracle)
    E = len(kind)
    used = int(g[f"loop{si}/variates_used"])
    normals = np.random.RandomState(int(g[f"loop{si}/np_seed"])).standard_normal(used + 64)
    models, model_of = mixed_model_rows(g, si, oracle)
    p = f"loop{si}/dt30"
    o = oracle.rollout(**sc, kind=kind, dt=1 / 30, ctrl=ctrl, route_off=roff, routes=routes, models=models, model_of=model_of,
                       noise=dict(mode="stream", std_lon=0.0, std_lat=0.0, normals=normals))
    assert o["n_steps"] == int(g[p + "/n_steps"]) and bits_equal(o["t"], g[p + "/t"])
    assert o["noise_used"] == used
    for k in ("poses", "vels", "dists"):
        assert np.array_equal(np.isnan(o[k]), np.isnan(g[p + "/" + k]))
        assert np.nanmax(np.abs(o[k] - g[p + "/" + k])) < PED_TOL, (p, k)
    ex = g[p + "/extra"]
    ped = ~np.isnan(ex[0, :, 0])
    assert np.array_equal(o["extra"][:, ped, 1], ex[:, ped, 1])              # goal_idx exact
    assert np.abs(o["extra"][:, ped] - ex[:, ped]).max() < PED_TOL           # controller speed; force
    rw = ped & (models[model_of, 0] == 1)
    assert not ex[:, rw, 2:].any() and not o["extra"][:, rw, 2:].any()       # RandomWalk never touches agent.force
    assert np.abs(ex[:, ped & ~rw, 2:]).max() > 0.1                          # ... the SocialForce pedestrians do feel one
    assert np.array_equal(oracle.coll_to_dense(o["coll"], E), g[p + "/coll"])
    assert np.array_equal(o["ev_t"], g[p + "/ev_t"]) and np.array_equal(o["ev_other"], g[p + "/ev_other"])
    # one model for everybody walks elsewhere (the test would pass trivially otherwise)
    o0 = oracle.rollout(**sc, kind=kind, dt=1 / 30, ctrl=ctrl, route_off=roff, routes=routes, sf=models[0, 1:13],
                        noise=dict(mode="stream", std_lon=models[0, 13], std_lat=models[0, 14], normals=normals))
    n = min(o0["n_steps"], o["n_steps"]) + 1
    assert np.nanmax(np.abs(o0["poses"][:n] - o["poses"][:n])) > 1e-3


# ---------------------------------------------------------------- the headline horizons on the reference itself (long.npz)
LONG_TOL = 1e-5  # the contract for controller-integrated poses (north_star); measured maxima are asserted far below it


def long_c3_batch(tracking=False):
    """Scenarios 0 and 1 of the bench's c3 family (the generator call of tests/golden/make_golden_long.py), PID egos, every
    entity's knots passed through Trajectory.__init__ as the reference does when it builds the scenario (trajectory.py:34-96
    re-sums the headings: scenario_gym_amd.trajectory.Trajectory, row T3) -- checked against the fixture's checksums of both."""
    import hashlib

    from scenario_gym_amd import _lib as L
    from scenario_gym_amd import synthetic
    from scenario_gym_amd.packing import unpack_scenario
    from scenario_gym_amd.trajectory import Trajectory

    packed = synthetic.make_batch(2, 64, n_steps=10000, timestep=1.0 / 30.0, ego_kind=L.KIND_AGENT_PID)
    g = load_golden("long")
    E = 64
    for k in (0, 1):  # the fixture was recorded on exactly these knots
        s = unpack_scenario(packed, k)
        d = hashlib.sha256(np.ascontiguousarray(s["knots"]).tobytes() + np.ascontiguousarray(s["knot_off"]).tobytes()
                           + np.ascontiguousarray(s["bbox"]).tobytes()).digest()
        assert np.array_equal(np.frombuffer(d, np.uint8), g[f"c3/{k}/knots_sha256"]), k
    changed = 0
    for i in range(2 * E):
        a, b = packed.knot_off[i], packed.knot_off[i + 1]
        data = Trajectory(packed.knots[a:b]).data
        assert data.shape == (b - a, 7)
        changed += int((data != packed.knots[a:b]).sum())
        packed.knots[a:b] = data
    assert changed > 0  # (the constructor is not the identity on these headings: an ulp here and there)
    for k in (0, 1):
        a, b = packed.knot_off[k * E], packed.knot_off[(k + 1) * E]
        d = hashlib.sha256(np.ascontiguousarray(packed.knots[a:b]).tobytes()).digest()
        assert np.array_equal(np.frombuffer(d, np.uint8), g[f"c3/{k}/trajectory_data_sha256"]), k  # == the reference's Trajectory.data
    if tracking:  # the PID gains of the reference's own controller test (tests/test_controller.py:7-25), as make_golden_long's c3t
        for k in (0, 1):
            packed.ctrl[k * E, L.C_ACCEL_KP], packed.ctrl[k * E, L.C_MAX_ACCEL], packed.ctrl[k * E, L.C_MAX_STEER] = 2.0, 5.0, np.pi / 90
    return packed.validate(), g


def check_long_c3t(g, k, n_steps, t, ego_poses, ego_extra, final_poses, final_vels, final_dists, metrics):
    """c3t: the same scenario with a PID loop that tracks (the reference's one-ulp twin stays within 1e-12 over the whole
    horizon).  Every step of all 10,000 within the contract -- far inside it --, replay lanes and clock bit for bit, the three
    ego metrics.  Returns the largest ego deviation."""
    p = f"c3t/{k}"
    assert n_steps == int(g[p + "/n_steps"]) >= 9999 and bits_equal(t, g[p + "/t"])
    assert g[p + "/self_divergence"].max() < 1e-11
    ref = g[p + "/ego"]
    err = float(np.abs(ego_poses - ref[:, :6]).max())
    if ego_extra is not None:
        err = max(err, float(np.abs(ego_extra - ref[:, 6:10]).max()))
    assert err < LONG_TOL, err
    fp, fv, fd = g[p + "/final_poses"], g[p + "/final_vels"], g[p + "/final_dists"]
    assert bits_equal(final_poses[1:], fp[1:]) and bits_equal(final_vels[1:], fv[1:]) and bits_equal(final_dists[1:], fd[1:])
    assert np.abs(final_poses[0] - fp[0]).max() < LONG_TOL and np.abs(final_vels[0] - fv[0]).max() < LONG_TOL and abs(final_dists[0] - fd[0]) < LONG_TOL
    for name in ("ego_avg_speed", "ego_max_speed", "ego_distance_travelled"):
        assert abs(metrics[name] - float(g[f"{p}/metric_{name}"])) < LONG_TOL, name
    return err


@pytest.mark.parametrize("k", [0, 1])
def test_headline_horizon_with_a_tracking_pid_matches_reference(oracle, k):
    """The 1e-5 contract for controller-integrated poses over config 3's FULL horizon, where it is well-posed: the bench's
    scenarios with the PID gains of the reference's own controller test (the loop tracks; the reference's one-ulp twin stays
    within 1e-12).  10,000 steps of the real reference: the oracle's ego pose and controller state after every step, the final
    state of all 64 entities and the three ego metrics."""
    from scenario_gym_amd.packing import unpack_scenario

    packed, g = long_c3_batch(tracking=True)
    s = unpack_scenario(packed, k)
    o = oracle.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], s["kind"], s["ego"], s["t0"], s["length"], 1.0 / 30.0,
                       ctrl=s["ctrl"], max_steps=10005)
    err = check_long_c3t(g, k, o["n_steps"], o["t"], o["poses"][:, 0], o["extra"][:, 0], o["poses"][-1], o["vels"][-1], o["dists"][-1],
                         {n: o["metric_" + n] for n in ("ego_avg_speed", "ego_max_speed", "ego_distance_travelled")})
    assert err < 1e-8, err
    print(f"c3t/{k}: max |ego pose / controller state - reference| over 10,000 steps = {err:.3e}")


def check_long_c3(g, k, n_steps, t, ego_poses, ego_extra, final_poses, final_vels, final_dists):
    """One c3 scenario after its 10,000 steps against the reference's record.  The clock and every replay lane: bit for bit.
    The PID ego: this closed loop amplifies a rounding error by ten every ~100 steps -- the fixture holds how far the reference
    drifts from ITSELF when its ego starts one ulp to the side (`self_divergence`: 1e-5 after 1,384 / 756 steps, metres after
    1,600) -- so the 1e-5 contract is checked on every step up to the last one at which the reference's own twin is still
    within 1e-7, and from there on the error may grow no faster than the twin's does.  Returns (largest error on the checked
    prefix, its length, the first step at which the error exceeds 1e-5 or None)."""
    p = f"c3/{k}"
    assert n_steps == int(g[p + "/n_steps"]) >= 9999 and bits_equal(t, g[p + "/t"])  # (max_length ends the 10,000-step scenario after 9,999: t + dt > length)
    ref, twin = g[p + "/ego"], g[p + "/self_divergence"]
    err = np.abs(ego_poses - ref[:, :6]).max(axis=1)
    if ego_extra is not None:
        err = np.maximum(err, np.abs(ego_extra - ref[:, 6:10]).max(axis=1))
    prefix = int(np.argmax(twin > 1e-7))  # (the twin does leave the band: asserted by the fixture's own numbers below)
    assert 500 < prefix < 2000 and twin.max() > 1.0
    assert err[:prefix].max() < LONG_TOL, (k, float(err[:prefix].max()))
    # ... and no faster than the reference's own sensitivity from there on (three decades of allowance)
    assert (err[prefix:] <= 1e3 * np.maximum(np.maximum.accumulate(twin)[prefix:], 1e-7)).all()
    fp, fv, fd = g[p + "/final_poses"], g[p + "/final_vels"], g[p + "/final_dists"]
    assert np.array_equal(np.isnan(final_poses), np.isnan(fp))
    assert bits_equal(final_poses[1:], fp[1:]) and bits_equal(final_vels[1:], fv[1:]) and bits_equal(final_dists[1:], fd[1:])
    over = np.argmax(err > LONG_TOL)
    return float(err[:prefix].max()), prefix, (int(over) if err[over] > LONG_TOL else None)


@pytest.mark.parametrize("k", [0, 1])
def test_headline_horizon_pid_ego_matches_reference(oracle, k):
    """BASELINE config 3 at its own length: 64 entities, the reference's PIDAgent on the ego, 10,000 steps of 1/30 s, recorded
    from the real reference.  The oracle reproduces the clock and every replay lane bit for bit over the whole horizon; the
    ego within 1e-5 for as long as the reference agrees with its own one-ulp twin (see check_long_c3)."""
    from scenario_gym_amd.packing import unpack_scenario

    packed, g = long_c3_batch()
    s = unpack_scenario(packed, k)
    o = oracle.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], s["kind"], s["ego"], s["t0"], s["length"], 1.0 / 30.0,
                       ctrl=s["ctrl"], max_steps=10005)
    err, prefix, over = check_long_c3(g, k, o["n_steps"], o["t"], o["poses"][:, 0], o["extra"][:, 0], o["poses"][-1], o["vels"][-1], o["dists"][-1])
    twin = g[f"c3/{k}/self_divergence"]
    print(f"c3/{k}: max |ego - reference| on the first {prefix} steps = {err:.3e}; exceeds 1e-5 at step {over}; "
          f"the reference's own one-ulp twin exceeds 1e-5 at step {int(np.argmax(twin > 1e-5))}")


def long_crowd_inputs(g, k, oracle):
    sc = scenario_arrays(g, f"crowd/{k}/scenario")
    E = len(sc["etype"])
    ctrl = np.tile(oracle.DEFAULT_CTRL, (E, 1))
    ctrl[:, 9], ctrl[:, 12] = g[f"crowd/{k}/vdes"], float(g[f"crowd/{k}/distance_threshold"])
    kind = np.full(E, oracle.KIND_AGENT_PEDESTRIAN, np.int32)
    nw = g[f"crowd/{k}/routes"].shape[1]
    return sc, kind, ctrl, np.arange(E + 1, dtype=np.int64) * nw, g[f"crowd/{k}/routes"].reshape(-1, 2)


def check_long_crowd(g, k, n_steps, t, poses, final_vels, final_dists, final_extra, coll_dense, ev_t, ev_other, tol=LONG_TOL):
    """poses [n + 1][E][6].  Returns the largest pose deviation."""
    p = f"crowd/{k}"
    assert n_steps == int(g[p + "/n_steps"]) >= 3299 and bits_equal(t, g[p + "/t"])
    traced = (0, 7, 19, 31)
    err = max(float(np.abs(poses[:, list(traced)] - g[p + "/traced"]).max()), float(np.abs(poses[::25] - g[p + "/poses_every25"]).max()),
              float(np.abs(poses[-1] - g[p + "/final_poses"]).max()))
    assert err < tol, err
    assert np.abs(final_vels - g[p + "/final_vels"]).max() < 1e-4 and np.abs(final_dists - g[p + "/final_dists"]).max() < 1e-4
    ex = g[p + "/final_extra"]
    assert np.array_equal(final_extra[:, 1], ex[:, 1]) and np.abs(final_extra - ex).max() < 1e-4  # goal index exact
    assert np.array_equal(coll_dense, g[p + "/final_coll"])
    assert np.array_equal(ev_t, g[p + "/ev_t"]) and np.array_equal(ev_other, g[p + "/ev_other"])
    return err


@pytest.mark.parametrize("k", [0, 1])
def test_long_crowd_matches_reference(oracle, k):
    """32 pedestrians that meet in the middle of a 12 m square, 3,300 steps (a third of config 5's horizon, ten times the
    closed loops of pedestrian.npz) from the real reference: without noise, and with the reference's noise drawn from numpy's
    global stream.  Poses within the contract at every recorded step, goal indices, the final adjacency and the ego's
    collision events exact, the same number of variates consumed."""
    g = load_golden("long")
    sc, kind, ctrl, roff, routes = long_crowd_inputs(g, k, oracle)
    std_lon, std_lat, seed = g[f"crowd/{k}/noise"]
    noise = None
    if std_lon or std_lat:
        used = int(g[f"crowd/{k}/variates_used"])
        noise = dict(mode="stream", std_lon=std_lon, std_lat=std_lat, normals=np.random.RandomState(int(seed)).standard_normal(used + 64))
    o = oracle.rollout(**sc, kind=kind, dt=1.0 / 30.0, ctrl=ctrl, route_off=roff, routes=routes, noise=noise, max_steps=3305, event_cap=512)
    if noise:
        assert o["noise_used"] == used
    err = check_long_crowd(g, k, o["n_steps"], o["t"], o["poses"], o["vels"][-1], o["dists"][-1], o["extra"][-1],
                           oracle.coll_to_dense(o["coll"], len(kind))[-1], o["ev_t"], o["ev_other"])
    print(f"crowd/{k}: max |pose - reference| over 3,300 steps = {err:.3e}")


def test_counter_based_noise_generator(oracle):
    """The timing-run generator (noise mode "device": Philox4x32-10 + Box-Muller with the shared log / sin / cos): standard
    normal moments over 2 x 10^5 variates, no correlation between the two outputs, different streams per scenario, and
    log within 1 ulp of libm."""
    import math

    z = np.array([oracle.noise_pair(2024, s, e, k) for s in range(8) for e in range(64) for k in range(200)])
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and abs(np.corrcoef(z.T)[0, 1]) < 0.01
    assert abs((z ** 3).mean()) < 0.03 and abs((z ** 4).mean() - 3.0) < 0.1
    assert not np.array_equal(oracle.noise_pair(1, 0, 3, 5), oracle.noise_pair(1, 1, 3, 5))
    assert np.array_equal(oracle.noise_pair(1, 0, 3, 5), oracle.noise_pair(1, 0, 3, 5))
    for x in np.concatenate([np.random.default_rng(0).uniform(1e-16, 1, 3000), np.random.default_rng(1).uniform(0.5, 2, 3000)]):
        assert abs(oracle.log(x) - math.log(x)) <= np.spacing(abs(math.log(x)))


def test_every_fixture_has_a_generator_and_is_not_older_than_it():
    """Every .npz under tests/golden/ is written by exactly one committed generator (tools/regen_golden.py's table), and no
    generator has been committed after the fixture it writes without the fixture being regenerated: compared by the git commit
    times of the two files (skipped outside a git checkout, e.g. on the GPU box's snapshot)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import regen_golden

    here = os.path.join(root, "tests", "golden")
    stems = sorted(f[:-4] for f in os.listdir(here) if f.endswith(".npz"))
    owned = sorted(s for v in regen_golden.GENERATORS.values() for s in v)
    assert stems == owned
    for g in regen_golden.GENERATORS:
        assert os.path.exists(os.path.join(here, g + ".py")), g
    if not os.path.isdir(os.path.join(root, ".git")):
        pytest.skip("not a git checkout")

    def committed(path):
        out = subprocess.run(["git", "log", "-1", "--format=%ct", "--", path], cwd=root, capture_output=True, text=True)
        return int(out.stdout.strip() or 0)

    for g, files in regen_golden.GENERATORS.items():
        tg = committed(os.path.join("tests", "golden", g + ".py"))
        for stem in files:
            tf = committed(os.path.join("tests", "golden", stem + ".npz"))
            # (a generator edit that does not change its output -- a comment, the SG_GOLDEN_OUT switch -- is committed together
            # with a regeneration check: the fixture's commit is then older, which the per-generator allowance below records)
            assert tf >= tg or (g, stem) in GENERATOR_EDITS_WITHOUT_OUTPUT_CHANGE, (g, stem, tg, tf)


# (generator, fixture) pairs whose generator was touched after the fixture with output verified unchanged by
# tools/regen_golden.py (3241 / 3241 on the round-5 tree: profiles/r05_regen_golden.txt)
GENERATOR_EDITS_WITHOUT_OUTPUT_CHANGE = {
    (g, s) for g, ss in {
        "make_golden": ["trajectory", "batch", "scenarios", "synth", "pid_xosc", "collision", "pedestrian"],
        "make_golden_actions": ["actions"], "make_golden_all_scenarios": ["all_scenarios"],
        "make_golden_collision_types": ["collision_types"], "make_golden_json": ["json", "elevation"],
        "make_golden_ped_noise": ["ped_noise"], "make_golden_random_walk": ["random_walk"], "make_golden_roads": ["roads"],
        "make_golden_rss": ["rss"], "make_golden_sensors": ["sensors"],
    }.items() for s in ss
}
