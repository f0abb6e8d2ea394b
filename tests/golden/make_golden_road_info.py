#!/usr/bin/env python3
"""Golden vectors for the per-geometry road query (N6 `State.get_road_info_at_entity` /
`RoadNetwork.get_geometries_at_point`, state/state.py:330-338, road_network/road_network.py:375-407) from the REAL
reference: tests/golden/road_info.npz.

Build container only (needs /root/reference and the import stand-ins of tests/golden/_refstubs, see its README):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_road_info.py

What comes from the reference: the geometries of each network, their classes, the lanes' parents, the loop over
`road_network_geometries`, the gym loop and `state.poses`.  `x.boundary.contains(Point)` is the stand-in's crossing number
of that one polygon's rings, exact for the fp64 coordinates given; nothing is dissolved here, so unlike the union layers
of make_golden_roads there is no shared-edge caveat: this is GEOS's answer for every point, on-ring points included.

The reference walks its lanes in a per-process hash order, so every answer is stored sorted by (class rank, id): a fixture
must come out the same every time it is regenerated.  The query points are those of roads.npz (`net/<name>/points`), which
this script reads; only the answers are stored here.  Only data is stored.
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path[:0] = [os.path.join(HERE, "_refstubs"), "/root/reference"]

import numpy as np  # noqa: E402

import scenario_gym  # noqa: E402
from scenario_gym import ScenarioGym  # noqa: E402
from scenario_gym.road_network import RoadNetwork  # noqa: E402
from scenario_gym.xosc_interface import import_scenario  # noqa: E402

assert scenario_gym.__version__ == "0.3.1"
SCEN_DIR = "/root/reference/tests/input_files/Scenarios"
NET_DIR = "/root/reference/tests/input_files/Road_Networks"
CLASSES = ["Road", "Intersection", "Lane", "Pavement", "Crossing", "Building"]
STATE_INFO = "3e39a079-5653-440c-bcbe-24dc9f6bf0e6"  # the fixture scenario of tests/test_state.py


def answer(names, geoms):
    """One reference answer -> [(class name, id)] sorted by (class rank, id)."""
    return sorted(((n, g.id) for n, g in zip(names, geoms)), key=lambda a: (CLASSES.index(a[0]), a[1]))


def csr(out, key, answers):
    """answers: list of [(class name, id)] -> <key>/off [n + 1], <key>/ids, <key>/names (flat, in answer order)."""
    out[f"{key}/off"] = np.concatenate([[0], np.cumsum([len(a) for a in answers])]).astype(np.int64)
    flat = [x for a in answers for x in a]
    out[f"{key}/names"] = np.array([x[0] for x in flat], dtype="U12")
    out[f"{key}/ids"] = np.array([x[1] for x in flat], dtype="U64")
    assert all(len(x[1]) <= 64 for x in flat)


def main():
    out = {}
    roads = np.load(os.path.join(HERE, "roads.npz"))
    nets = [str(n) for n in roads["networks"]]
    assert nets == sorted(f[:-5] for f in os.listdir(NET_DIR) if f.endswith(".json"))
    out["classes"] = np.array(CLASSES)
    for n in nets:
        rn = RoadNetwork.create_from_json(os.path.join(NET_DIR, n + ".json"))
        geoms = {g.id: g for g in rn.road_network_geometries}
        ids = [str(i) for i in roads[f"net/{n}/ids"]]
        assert sorted(geoms) == ids and len(rn.road_network_geometries) == len(ids)  # ids are unique within the network
        # class of every polygon of roads.npz (its order: sorted by id) and the id of each lane's parent ("" = free-standing)
        out[f"net/{n}/classes"] = np.array([type(geoms[i]).__name__ for i in ids], dtype="U12")
        parents = []
        for i in ids:
            p = rn.get_lane_parent(geoms[i]) if type(geoms[i]).__name__ == "Lane" else None
            parents.append("" if p is None else p.id)
        out[f"net/{n}/lane_parent"] = np.array(parents, dtype="U64")
        pts = roads[f"net/{n}/points"]
        t0 = time.time()
        answers = [answer(*rn.get_geometries_at_point(float(x), float(y))) for x, y in pts]
        dt = time.time() - t0
        csr(out, f"net/{n}", answers)
        print(n, len(ids), "geometries,", len(pts), "points,", "%.2f ms per point," % (1e3 * dt / len(pts)),
              "largest answer", max(len(a) for a in answers), "non-empty", sum(1 for a in answers if a))

    # ---- State.get_road_info_at_entity along the rollouts of roads.npz: step 0 and every 30th step ----
    names = [str(n) for n in roads["scenarios"]]
    for n in names:
        s = import_scenario(os.path.join(SCEN_DIR, n + ".xosc"))
        assert s.road_network.name == str(roads[f"{n}/network"])
        gym = ScenarioGym(timestep=0.1)
        gym.set_scenario(s)
        ents = gym.state.scenario.entities
        assert [e.ref for e in ents] == [str(r) for r in roads[f"{n}/scenario/refs"]]
        steps, present, answers = [], [], []

        def frame(k):
            steps.append(k)
            poses = gym.state.poses
            present.append([e in poses for e in ents])
            for e in ents:
                answers.append(answer(*gym.state.get_road_info_at_entity(e)) if e in poses else [])

        frame(0)
        k = 0
        while not gym.state.is_done:
            gym.step()
            k += 1
            if k % 30 == 0:
                frame(k)
        out[f"{n}/steps"] = np.array(steps, np.int64)
        out[f"{n}/present"] = np.array(present, np.uint8)  # [frames][entities]
        csr(out, n, answers)                               # row = frame * n_entities + entity
        print(n, s.road_network.name, len(steps), "frames,", int(np.sum(present)), "answers,", sum(len(a) for a in answers), "geometries")

    # ---- tests/test_state.py:74-100 (test_state_info): 50 steps at 0.1 s, the road info of entities[0] ----
    s = import_scenario(os.path.join(SCEN_DIR, STATE_INFO + ".xosc"))
    gym = ScenarioGym(timestep=0.1)
    gym.set_scenario(s)
    for _ in range(50):
        gym.step()
    e = gym.state.scenario.entities[0]
    got_names, got_geoms = gym.state.get_road_info_at_entity(e)
    assert "Road" in got_names
    a = answer(got_names, got_geoms)
    out["state_info/scenario"] = np.array(STATE_INFO)
    out["state_info/network"] = np.array(s.road_network.name)
    out["state_info/entity"] = np.array(e.ref)
    out["state_info/names"] = np.array([x[0] for x in a], dtype="U12")
    out["state_info/ids"] = np.array([x[1] for x in a], dtype="U64")
    print("state_info", s.road_network.name, e.ref, a)
    np.savez_compressed(os.path.join(os.environ.get("SG_GOLDEN_OUT", HERE), "road_info.npz"), **out)


if __name__ == "__main__":
    main()
