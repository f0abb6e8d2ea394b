"""Which road geometries contain each entity / each point: State.get_road_info_at_entity (state/state.py:330-338)
and RoadNetwork.get_geometries_at_point (road_network/road_network.py:375-407) on the device -- sg_road_info,
sg_road_info_points -- against the real reference's answers (tests/golden/road_info.npz), and the host-only lane graph
(road_network.py:330-373).  The GPU tests go through the C ABI and read only tests/golden/."""
import json
import os

import numpy as np
import pytest

from conftest import load_golden, scenario_arrays
from road_shapes import _contains_all, _edges_of
from test_host_api import scenario_from_arrays

gpu = pytest.mark.gpu
RANK = {n: k for k, n in enumerate(["Road", "Intersection", "Lane", "Pavement", "Crossing", "Building"])}
SIX_LANE = "dRisk Unity 6-lane Intersection"


def _nets(g):
    return [str(n) for n in g["networks"]]


def _arrays(g, net):
    return {k: g[f"net/{net}/{k}"] for k in ("ring_off", "vert_off", "verts", "layers")}


def _expected(g, ri, net):
    """Per fixture point of `net`: the ascending polygon indices (roads.npz order) the reference's answer names."""
    pos = {str(i): k for k, i in enumerate(g[f"net/{net}/ids"])}
    off, ids = ri[f"net/{net}/off"], ri[f"net/{net}/ids"]
    return [sorted(pos[str(i)] for i in ids[off[k]:off[k + 1]]) for k in range(len(off) - 1)]


def _rows(count, geoms):
    return [list(g[:max(c, 0)]) for c, g in zip(count.ravel(), geoms.reshape(count.size, -1))]


def _batch_on_networks(g, nets, R, E, n_steps=200, seed=5):
    """A synthetic batch whose scenario r roams the extent of network nets[r % len(nets)]: (packed, arrays, net_of)."""
    from scenario_gym_amd import synthetic

    arrs = [_arrays(g, n) for n in nets]
    net_of = np.arange(R) % len(nets)
    half = min(float((a["verts"].max(0) - a["verts"].min(0)).min()) for a in arrs) / 2
    packed = synthetic.make_batch(R, E, n_steps=n_steps, timestep=0.1, n_knots=16, extent=half, vanish_frac=0.3, seed=seed)
    for r in range(R):
        v = arrs[net_of[r]]["verts"]
        a, b = packed.knot_off[r * E], packed.knot_off[(r + 1) * E]
        packed.knots[a:b, 1:3] += (v.max(0) + v.min(0)) / 2
    return packed, arrs, net_of


def _engine(sga, g, nets, R, E, **kw):
    packed, arrs, net_of = _batch_on_networks(g, nets, R, E, **kw)
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks(arrs, net_of)
    return eng, arrs, net_of


@pytest.fixture
def sga():
    import scenario_gym_amd as sga

    return sga


# ---------------------------------------------------------------- CPU: the fixture, the lane graph, the index -> object map
def test_fixture_answers_are_the_exact_crossing_number():
    """Every answer of road_info.npz, all six networks and all their points (uniform, on vertices, 1e-9 beside vertices, edge
    midpoints), recomputed from the rings of roads.npz: strictly inside the exterior ring and outside the holes, on a ring =
    not contained, decided in exact rational arithmetic where fp64 could be in doubt.  No point is left out."""
    g, ri = load_golden("roads"), load_golden("road_info")
    assert [str(c) for c in ri["classes"]] == list(RANK)
    total = hits = 0
    for net in _nets(g):
        edges, off = _edges_of(_arrays(g, net))
        want = _expected(g, ri, net)
        pts = g[f"net/{net}/points"]
        assert len(want) == len(pts)
        for (px, py), w in zip(pts, want):
            assert list(np.nonzero(_contains_all(edges, off, px, py))[0]) == w, (net, px, py)
            hits += len(w)
        total += len(pts)
        # stored sorted by (class rank, id), classes consistent with the network's
        cls = {str(i): str(c) for i, c in zip(g[f"net/{net}/ids"], ri[f"net/{net}/classes"])}
        o, ids, names = ri[f"net/{net}/off"], ri[f"net/{net}/ids"], ri[f"net/{net}/names"]
        for k in range(len(o) - 1):
            a = [(RANK[str(n)], str(i)) for n, i in zip(names[o[k]:o[k + 1]], ids[o[k]:o[k + 1]])]
            assert a == sorted(a) and all(cls[i] == list(RANK)[r] for r, i in a)
    assert total == 13800 and hits > 20000


def test_lane_graph_and_geometry_index(reference_inputs):
    """road_network.py:330-373 on the six networks: object_by_id, driveable_lanes, successors / predecessors, connecting roads
    <-> intersections, the lanes' parents (against the reference's get_lane_parent, road_info.npz), also after a to_dict round
    trip; and polygon k of polygon_arrays() is geometry k of geometry_index()."""
    from scenario_gym_amd.road_network import Lane, RoadNetwork

    g, ri = load_golden("roads"), load_golden("road_info")
    n_succ = n_conn = 0
    for net in _nets(g):
        rn = RoadNetwork.create_from_json(os.path.join(reference_inputs, "Road_Networks", net + ".json"))
        for rn in (rn, RoadNetwork.create_from_dict(rn.to_dict())):
            geoms = rn.geometry_index()
            assert [x.id for x in geoms] == [str(i) for i in rn.polygon_arrays()["ids"]] and geoms == rn.road_network_geometries
            assert sorted(x.id for x in geoms) == [str(i) for i in g[f"net/{net}/ids"]]
            cls = {str(i): str(c) for i, c in zip(g[f"net/{net}/ids"], ri[f"net/{net}/classes"])}
            parent = {str(i): str(p) for i, p in zip(g[f"net/{net}/ids"], ri[f"net/{net}/lane_parent"])}
            lanes = {l.id: l for l in rn.lanes}
            for x in geoms:
                assert rn.object_by_id(x.id) is x and type(x).__name__ == cls[x.id]
            assert rn.driveable_lanes == [l for l in rn.lanes if l.type == "driving"]
            for l in rn.lanes:
                assert isinstance(l, Lane)
                p = rn.get_lane_parent(l)
                assert ("" if p is None else p.id) == parent[l.id] and (p is None or l in p.lanes)
                succ, pred = rn.get_successor_lanes(l), rn.get_predecessor_lanes(l)
                assert [s.id for s in succ] == l.successors and [s.id for s in pred] == l.predecessors
                assert all(lanes[s.id] is s for s in succ + pred)
                n_succ += len(succ)
            for i in rn.intersections:
                roads = rn.get_connecting_roads(i)
                assert {r.id for r in roads} == set(i.connecting_roads) & {r.id for r in rn.roads}
                assert all(i in rn.get_intersections(r) for r in roads)
                n_conn += len(roads)
            for r in rn.roads:
                assert all(r in rn.get_connecting_roads(i) for i in rn.get_intersections(r))
    assert n_succ > 50 and n_conn > 10


# ---------------------------------------------------------------- GPU
@gpu
def test_points_match_the_reference(sga):
    """1. All six networks as one batch of six scenarios; sg_road_info_points on every fixture point: the reference's id sets
    exactly (0 mismatches), ascending indices, count = the set's size, layers = the OR of the polygons' bits."""
    g, ri = load_golden("roads"), load_golden("road_info")
    nets = _nets(g)
    eng, arrs, _ = _engine(sga, g, nets, len(nets), 4)
    pts = np.concatenate([g[f"net/{n}/points"] for n in nets])
    scen = np.concatenate([np.full(len(g[f"net/{n}/points"]), k, np.int32) for k, n in enumerate(nets)])
    want = [w for n in nets for w in _expected(g, ri, n)]
    cap = 32
    count, layers = np.full(len(pts), -7, np.int32), np.zeros(len(pts), np.uint32)
    geoms = np.full((len(pts), cap), -7, np.int32)
    rc = eng.lib.sg_road_info_points(eng.h, len(pts), scen.ctypes.data, pts.ctypes.data, cap, count.ctypes.data, geoms.ctypes.data,
                                     layers.ctypes.data)
    assert rc == 0
    bad = [k for k in range(len(pts)) if count[k] != len(want[k]) or list(geoms[k, :count[k]]) != want[k]]
    assert bad == [] and len(pts) == 13800
    assert all((geoms[k, count[k]:] == -1).all() for k in range(len(pts)))
    for k in range(len(pts)):
        assert layers[k] == np.bitwise_or.reduce(arrs[scen[k]]["layers"][want[k]], initial=0)
    assert max(len(w) for w in want) > 20 and eng.road_info_points(scen, pts)[0].tolist() == count.tolist()
    eng.close()


def _sorted_answer(names, objs):
    return sorted(((n, o.id) for n, o in zip(names, objs)), key=lambda a: (RANK[a[0]], a[1]))


@gpu
def test_entities_match_the_reference_along_rollouts(sga, reference_inputs):
    """2. State.get_road_info_at_entity (names and objects) of every entity in state.poses at step 0 and every 30th step of the
    four reference rollouts of roads.npz; KeyError for an entity that is not in the scene; the last two lines of the
    reference's test_state_info (tests/test_state.py:99-100) on its own scenario."""
    from scenario_gym_amd.road_network import RoadNetwork
    from scenario_gym_amd.scenario import Scenario

    g, ri = load_golden("roads"), load_golden("road_info")
    net = lambda name: RoadNetwork.create_from_json(os.path.join(reference_inputs, "Road_Networks", name + ".json"))  # noqa: E731
    answers = absent = 0
    for n in (str(x) for x in g["scenarios"]):
        sc = scenario_from_arrays(scenario_arrays(g, f"{n}/scenario"), g[f"{n}/scenario/refs"])
        sc.road_network = rn = net(str(g[f"{n}/network"]))
        gym = sga.ScenarioGym(timestep=0.1)
        gym.set_scenario(sc)
        ents = gym.state.scenario.entities
        off, ids, names = ri[f"{n}/off"], ri[f"{n}/ids"], ri[f"{n}/names"]
        done = 0
        for f, step in enumerate(ri[f"{n}/steps"]):
            for _ in range(int(step) - done):
                gym.step()
            done = int(step)
            poses = gym.state.poses
            for k, e in enumerate(ents):
                assert (e in poses) == bool(ri[f"{n}/present"][f, k])
                if e not in poses:
                    with pytest.raises(KeyError):
                        gym.state.get_road_info_at_entity(e)
                    absent += 1
                    continue
                got_names, got = gym.state.get_road_info_at_entity(e)
                row = f * len(ents) + k
                want = list(zip((str(x) for x in names[off[row]:off[row + 1]]), (str(x) for x in ids[off[row]:off[row + 1]])))
                assert _sorted_answer(got_names, got) == want, (n, step, e.ref)
                order = [rn.geometry_index().index(o) for o in got]
                assert order == sorted(order) and all(rn.object_by_id(o.id) is o for o in got)
                answers += 1
        # the same call as a point query through the gym
        e0 = ents[0]
        if e0 in poses:
            assert gym.get_geometries_at_point(*poses[e0][:2])[1] == gym.state.get_road_info_at_entity(e0)[1]
        gym.close()
    assert answers > 100 and absent > 0
    # tests/test_state.py:74-100
    gj = load_golden("json")
    n = str(ri["state_info/scenario"])
    d = json.loads(str(gj[f"{n}/to_dict"]))
    for e in d["entities"]:
        e["trajectory"] = gj[f"{n}/traj_{e['trajectory']}"].tolist()
    d["road_network"] = None
    sc = Scenario.from_dict(d)
    sc.road_network = net(str(ri["state_info/network"]))
    gym = sga.ScenarioGym(timestep=0.1)
    gym.set_scenario(sc)
    for _ in range(50):
        gym.step()
    e = gym.state.scenario.entities[0]
    assert e.ref == str(ri["state_info/entity"])
    names, objs = gym.state.get_road_info_at_entity(e)
    assert "Road" in names, "Entity is on the road."
    assert _sorted_answer(names, objs) == list(zip((str(x) for x in ri["state_info/names"]), (str(x) for x in ri["state_info/ids"])))
    sc.road_network = None  # state.py:334-335
    gym.set_scenario(sc)
    assert gym.state.get_road_info_at_entity(gym.state.scenario.entities[0]) == ([], [])
    gym.close()


@gpu
def test_consistent_with_the_layer_index(sga):
    """3. 240 scenarios over all six networks, entities scattered over each network's extent, some of them gone: the ego's
    `layers & DRIVEABLE` is what ego_off_road and the centre cell of sg_raster_map say of the same pose; layers = the OR of
    poly_layers[geoms]; count == -1 exactly where SG_F_PRESENT is 0."""
    g = load_golden("roads")
    R, E = 240, 16
    eng, arrs, net_of = _engine(sga, g, _nets(g), R, E)
    on_road = 0
    for steps in (0, 45, 90):  # t = 0, 4.5 s (some entities not spawned yet), 13.5 s (some gone)
        eng.step(steps)
        st = eng.state()
        count, geoms, layers = eng.road_info()
        assert np.array_equal(count == -1, ~st["present"]) and (~st["present"]).any() and (count > 0).any()
        for r in range(R):
            L = arrs[net_of[r]]["layers"]
            for e in range(E):
                c = max(count[r, e], 0)
                assert layers[r, e] == np.bitwise_or.reduce(L[geoms[r, e, :c]], initial=0) and (geoms[r, e, c:] == -1).all()
        drive = (layers[:, 0] & 1) != 0
        assert np.array_equal(drive, (eng.terminal_flags() & 8) == 0)  # SG_TERM_EGO_OFF_ROAD of entities[0]
        centre = eng.raster_map([1], 0.0, 0.0, 1, 1)[:, 0, 0, 0]      # one cell at the ego's own position
        assert np.array_equal(drive & st["present"][:, 0], centre)
        on_road += int(drive.sum())
        pts = eng.road_info_points(np.repeat(np.arange(R), E), np.nan_to_num(st["poses"][:, :, :2]).reshape(-1, 2), cap=geoms.shape[2])
        ok = st["present"].ravel()
        assert np.array_equal(pts[0][ok], count.ravel()[ok]) and np.array_equal(pts[1][ok], geoms.reshape(R * E, -1)[ok])
    eng.close()
    assert on_road > 20


@gpu
@pytest.mark.parametrize("E", [16, 64, 300, 600])
def test_every_width_and_right_behind_a_rollout(sga, E):
    """4. 16, 64, 300 and 600 entity slots per scenario (one wavefront per scenario, several, the multi-kernel step): the
    answers for the entity slots are those of the point query at the same poses; and a query right behind sg_rollout_async,
    without a synchronize in between, sees the state the rollout leaves (it is ordered behind it on the handle's stream)."""
    g = load_golden("roads")
    R = 12
    eng, arrs, net_of = _engine(sga, g, _nets(g), R, E, n_steps=60)
    eng.rollout_async(40)
    count, geoms, layers = eng.road_info()     # no synchronize in between
    st = eng.state()
    assert (st["n_steps"] > 0).all()
    again = eng.road_info()
    assert all(np.array_equal(a, b) for a, b in zip((count, geoms, layers), again))
    ok = st["present"].ravel()
    pts = eng.road_info_points(np.repeat(np.arange(R), E), np.nan_to_num(st["poses"][:, :, :2]).reshape(-1, 2), cap=geoms.shape[2])
    assert np.array_equal(count.ravel() == -1, ~ok) and ok.sum() > R * E // 3
    assert np.array_equal(pts[0][ok], count.ravel()[ok]) and np.array_equal(pts[1][ok], geoms.reshape(R * E, -1)[ok])
    assert np.array_equal(pts[2][ok], layers.ravel()[ok]) and (count > 0).any()
    # device outputs: torch tensors the kernel writes directly
    tc, tg, tl = eng.road_info(cap=geoms.shape[2], torch_out=True)
    assert tc.is_cuda and tuple(tg.shape) == geoms.shape
    assert np.array_equal(tc.cpu().numpy(), count) and np.array_equal(tg.cpu().numpy(), geoms)
    assert np.array_equal(tl.cpu().numpy().view(np.uint32), layers)
    eng.close()


@gpu
def test_capacity(sga):
    """5. cap = 4 on the 6-lane intersection: true counts above 4, the first four indices, the layers of all; cap = 0 with NULL
    geoms: counts only; the Python wrapper re-queries and returns whole lists."""
    g, ri = load_golden("roads"), load_golden("road_info")
    eng, arrs, _ = _engine(sga, g, [SIX_LANE], 2, 4)
    want = _expected(g, ri, SIX_LANE)
    pts = np.ascontiguousarray(g[f"net/{SIX_LANE}/points"])
    n = len(pts)
    scen = np.ones(n, np.int32)
    count, layers, geoms = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.full((n, 4), -7, np.int32)
    assert eng.lib.sg_road_info_points(eng.h, n, scen.ctypes.data, pts.ctypes.data, 4, count.ctypes.data, geoms.ctypes.data, layers.ctypes.data) == 0
    assert count.tolist() == [len(w) for w in want] and count.max() > 20 and (count > 4).sum() > 100
    for k in range(n):
        assert list(geoms[k]) == (want[k] + [-1] * 4)[:4]
        assert layers[k] == np.bitwise_or.reduce(arrs[0]["layers"][want[k]], initial=0)
    only = np.zeros(n, np.int32)
    assert eng.lib.sg_road_info_points(eng.h, n, scen.ctypes.data, pts.ctypes.data, -5, only.ctypes.data, None, None) == 0  # cap ignored
    assert np.array_equal(only, count)
    c2, g2, _ = eng.road_info_points(scen, pts, cap=4)
    assert g2.shape[1] == count.max() and _rows(c2, g2) == want
    # the per-entity call: NULL geoms and layers
    ce = np.zeros((2, 4), np.int32)
    assert eng.lib.sg_road_info(eng.h, 0, ce.ctypes.data, None, None, 0) == 0
    assert np.array_equal(ce, eng.road_info(cap=1)[0])
    eng.close()


@gpu
def test_polygons_without_layer_bits_answer_too(sga):
    """6. A raw sg_road_networks whose polygons all appear a second time with layers = 0: the query names both copies (every
    polygon answers, whatever its bits), and the rasters and ego_off_road of that handle are those of a handle without them."""
    g = load_golden("roads")
    net = "Greenwich_Road_Network_002"
    a = _arrays(g, net)
    P = len(a["layers"])
    twice = dict(ring_off=np.concatenate([a["ring_off"], a["ring_off"][1:] + a["ring_off"][-1]]),
                 vert_off=np.concatenate([a["vert_off"], a["vert_off"][1:] + a["vert_off"][-1]]),
                 verts=np.concatenate([a["verts"], a["verts"]]), layers=np.concatenate([a["layers"], np.zeros(P, np.uint32)]))
    R, E = 24, 16
    packed, _, _ = _batch_on_networks(g, [net], R, E)
    out = []
    for arr in (a, twice):
        eng = sga.RolloutEngine(R, E, timestep=0.1)
        eng.upload(packed)
        eng.set_road_networks([arr], np.zeros(R, np.int32))
        eng.step(30)
        out.append((eng.road_info(), eng.raster_map([0, 1, 2, 4, 8, 16, 32, 64], 30.0, 30.0, 31, 31), eng.terminal_flags()))
        eng.close()
    (c1, g1, l1), map1, fl1 = out[0]
    (c2, g2, l2), map2, fl2 = out[1]
    assert np.array_equal(map1, map2) and np.array_equal(fl1, fl2) and map1[:, 1].any()
    assert np.array_equal(c2, np.where(c1 < 0, -1, 2 * c1)) and np.array_equal(l1, l2) and (c1 > 0).sum() > 5
    for x, y in zip(_rows(c1, g1), _rows(c2, g2)):
        assert y == x + [q + P for q in x]


@gpu
def test_errors_and_handles_without_networks(sga):
    """7. SG_ERR_STATE before sg_upload; SG_ERR_INVALID for cap < 0, a NULL count, NULL xy / scenario_of_point with n > 0 and a
    scenario index out of range; a handle on which sg_set_road_networks was never called answers 0 for every present entity."""
    from scenario_gym_amd import synthetic

    R, E = 8, 8
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    count, geoms = np.zeros((R, E), np.int32), np.zeros((R, E, 4), np.int32)
    xy, scen = np.zeros((3, 2)), np.zeros(3, np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert eng.lib.sg_road_info(eng.h, 4, p(count), p(geoms), None, 0) == -3
    assert eng.lib.sg_road_info_points(eng.h, 3, p(scen), p(xy), 4, p(count), p(geoms), None) == -3
    eng.upload(synthetic.make_batch(R, E, n_steps=100, timestep=0.1, vanish_frac=0.3))
    eng.step(10)
    assert eng.lib.sg_road_info(eng.h, -1, p(count), p(geoms), None, 0) == -1
    assert eng.lib.sg_road_info(eng.h, 4, None, p(geoms), None, 0) == -1
    assert b"sg_road_info" in eng.lib.sg_last_error(eng.h)
    assert eng.lib.sg_road_info_points(eng.h, 3, p(scen), p(xy), -1, p(count), p(geoms), None) == -1
    assert eng.lib.sg_road_info_points(eng.h, 3, p(scen), p(xy), 4, None, p(geoms), None) == -1
    assert eng.lib.sg_road_info_points(eng.h, 3, None, p(xy), 4, p(count), p(geoms), None) == -1
    assert eng.lib.sg_road_info_points(eng.h, 3, p(scen), None, 4, p(count), p(geoms), None) == -1
    assert eng.lib.sg_road_info_points(eng.h, -1, p(scen), p(xy), 4, p(count), p(geoms), None) == -1
    for bad in (-1, R):
        scen[1] = bad
        assert eng.lib.sg_road_info_points(eng.h, 3, p(scen), p(xy), 4, p(count), p(geoms), None) == -1
    assert eng.lib.sg_road_info_points(eng.h, 0, None, None, 4, p(count), p(geoms), None) == 0
    # no networks on the handle: the reference's ([], []) for a scenario without one
    c, gm, l = eng.road_info(cap=4)
    pres = eng.state()["present"]
    assert np.array_equal(c, np.where(pres, 0, -1)) and pres.any() and (~pres).any() and (gm == -1).all() and not l.any()
    assert not eng.road_info_points(np.zeros(3, np.int32), np.zeros((3, 2)))[0].any()
    # ... and a scenario with net_of_scenario = -1 beside one with a network
    g = load_golden("roads")
    a = _arrays(g, SIX_LANE)
    eng.set_road_networks([a], np.where(np.arange(R) % 2, 0, -1))
    mid = (a["verts"].max(0) + a["verts"].min(0)) / 2
    c, _, _ = eng.road_info_points(np.arange(R), np.tile(mid, (R, 1)))
    assert (c[0::2] == 0).all() and (c[1::2] > 0).all() and len(set(c[1::2])) == 1
    eng.close()


@gpu
def test_batched_gym_and_vector_env_views(sga, reference_inputs):
    """BatchedScenarioGym.road_info / get_geometries_at_points and VectorScenarioEnv.road_info (ego rows; torch tensors in
    HBM with torch_obs) against State.get_road_info_at_entity of the same scenarios."""
    from scenario_gym_amd.road_network import RoadNetwork

    g = load_golden("roads")
    scs = []
    for n in (str(x) for x in g["scenarios"]):
        sc = scenario_from_arrays(scenario_arrays(g, f"{n}/scenario"), g[f"{n}/scenario/refs"])
        sc.road_network = RoadNetwork.create_from_json(os.path.join(reference_inputs, "Road_Networks", str(g[f"{n}/network"]) + ".json"))
        scs.append(sc)
    gym = sga.BatchedScenarioGym(timestep=0.1)
    gym.set_scenarios(scs)
    gym.step(n=30)
    count, geoms, layers = gym.road_info()
    assert count.shape == geoms.shape[:2] == layers.shape and count.shape[0] == len(scs)
    ego_rows = []
    for i, sc in enumerate(scs):
        st = gym.states[i]
        for k, e in enumerate(sc.entities):
            if e in st.poses:
                names, objs = st.get_road_info_at_entity(e)
                assert [sc.road_network.geometry_index()[j] for j in geoms[i, k, :count[i, k]]] == objs
                assert gym.get_geometries_at_points(i, [st.poses[e][:2]])[0] == (names, objs)
            else:
                assert count[i, k] == -1
        assert (count[i, len(sc.entities):] == -1).all()  # padding slots
        k = sc.entities.index(sc.ego)
        ego_rows.append((count[i, k], list(geoms[i, k, :max(count[i, k], 0)]), layers[i, k]))
    gym.close()
    for torch_obs in (False, True):
        env = sga.VectorScenarioEnv(scs, timestep=0.1, n=8, terminal_conditions=["max_length"], torch_obs=torch_obs)
        env.reset()
        for _ in range(30):
            env.step(np.zeros((len(scs), 2)))
        c, gm, l = env.road_info()
        if torch_obs:
            assert c.is_cuda and gm.is_cuda and l.is_cuda
            c, gm, l = c.cpu().numpy(), gm.cpu().numpy(), l.cpu().numpy().view(np.uint32)
        assert c.shape == (len(scs),) and (c >= 0).all() and (l & 1).any()
        assert all((gm[i, c[i]:] == -1).all() for i in range(len(scs)))
        env.close()
    assert any(c > 0 for c, _, _ in ego_rows)
