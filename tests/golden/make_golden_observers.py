#!/usr/bin/env python3
"""Golden vectors for the observations of entities OTHER than the ego from the REAL reference:
tests/golden/observers.npz.

Build container only (needs /root/reference and the import stand-ins of tests/golden/_refstubs, see its README; the
collision predicates and `contains` come from the stand-ins' exact-rational tests on the reference's own fp64 coordinates):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_observers.py

For the shipped XOSC scenarios of sensors.npz that have a road network, rolled out by the reference at dt = 0.1, and for
at least three non-ego entities of each (one that spawns late or vanishes and one pedestrian / misc object where the
scenario has them, then by entity order):
  * FutureCollisionDetector(e, horizon) (sensor/common.py:60-106), horizons 5.0 and 1.0, on the state after reset and after
    every step -- whether or not `e` is in the scene, as the detector reads trajectories only;
  * RasterizedMapSensor(e, layers=[entity, driveable_surface, walkable_surface, lane]) (sensor/map.py:136-271) in the two
    grid configurations of sensors.npz on every 4th state in which `e` is in state.poses (the sensor reads state.poses[e]);
  * the step and entity indices, the poses of every entity on every 4th state, the scenario's arrays and its network's name
    (the polygons of every network are in roads.npz).
The oracle (oracle.raster_map / oracle.future_collision with the observer's index as `ego`) reproduces all recorded maps and
flags exactly: no grid point of these rollouts lies on an edge shared by two polygons of a union, the one case where the
stand-in's `contains` and the oracle's differ.  Only data is stored.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path[:0] = [os.path.join(HERE, "_refstubs"), "/root/reference"]

import numpy as np  # noqa: E402

import scenario_gym  # noqa: E402
from scenario_gym import ScenarioGym  # noqa: E402
from scenario_gym.sensor.common import FutureCollisionDetector  # noqa: E402
from scenario_gym.sensor.map import RasterizedMapSensor  # noqa: E402
from scenario_gym.xosc_interface import import_scenario  # noqa: E402

assert scenario_gym.__version__ == "0.3.1"
SCEN_DIR = "/root/reference/tests/input_files/Scenarios"
NAMES = ["a5e43fe4", "3fee6507", "41dac6fa", "5c5188e0", "a98d5c7d"]  # the scenarios of sensors.npz
ETYPE = {"Vehicle": 0, "Pedestrian": 1}
LAYERS = ["entity", "driveable_surface", "walkable_surface", "lane"]
EVERY = 4
N_OBSERVERS = 3


def export_scenario(out, key, s):
    ents = s.entities
    off = np.concatenate([[0], np.cumsum([e.trajectory.data.shape[0] for e in ents])]).astype(np.int64)
    out[f"{key}/scenario/knot_off"] = off
    out[f"{key}/scenario/knots"] = np.concatenate([e.trajectory.data for e in ents], axis=0)
    out[f"{key}/scenario/bbox"] = np.array([[e.bounding_box.width, e.bounding_box.length, e.bounding_box.center_x,
                                             e.bounding_box.center_y] for e in ents], np.float64)
    out[f"{key}/scenario/etype"] = np.array([ETYPE.get(e.catalog_entry.catalog_type, 2) for e in ents], np.int32)
    out[f"{key}/scenario/refs"] = np.array([e.ref for e in ents])
    out[f"{key}/scenario/ego"] = np.int64(ents.index(s.ego))
    out[f"{key}/scenario/length"] = np.float64(s.length)


def pick_observers(s, t0):
    """Indices of the non-ego entities that observe: one whose trajectory starts after the scenario does or ends before it,
    one that is no vehicle, then the others in entity order, N_OBSERVERS in all (fewer when the scenario has fewer)."""
    ents = s.entities
    others = [k for k, e in enumerate(ents) if e is not s.ego]
    partial = [k for k in others if ents[k].trajectory.min_t > t0 or ents[k].trajectory.max_t < s.length]
    soft = [k for k in others if ents[k].catalog_entry.catalog_type != "Vehicle"]
    chosen = []
    for k in partial[:1] + soft[:1] + others:
        if k not in chosen and len(chosen) < N_OBSERVERS:
            chosen.append(k)
    return sorted(chosen)


def main():
    out = {"horizons": np.array([5.0, 1.0]), "layers": np.array(LAYERS),
           # (width, height, n per side) as in sensors.npz: freq = 1 over 30 m x 30 m, and a fine 24 x 24 grid over 12 m x 12 m
           "raster_cfg": np.array([[30.0, 30.0, 30.0], [12.0, 12.0, 24.0]])}
    names = []
    for n in NAMES:
        path = [os.path.join(SCEN_DIR, f) for f in sorted(os.listdir(SCEN_DIR)) if f.startswith(n)][0]
        s = import_scenario(path)
        if s.road_network is None:
            continue
        names.append(n)
        gym = ScenarioGym(timestep=0.1)
        gym.set_scenario(s)
        ents = gym.state.scenario.entities
        export_scenario(out, n, gym.state.scenario)
        out[f"{n}/network"] = np.array(gym.state.scenario.road_network.name)
        obs = pick_observers(gym.state.scenario, gym.state.t)
        out[f"{n}/observers"] = np.array(obs, np.int64)
        detectors = [[FutureCollisionDetector(ents[k], horizon=h) for h in out["horizons"]] for k in obs]
        rasters = [[RasterizedMapSensor(ents[k], layers=LAYERS, width=w, height=h, freq=None, n=int(m), channels_first=True)
                    for w, h, m in out["raster_cfg"]] for k in obs]
        for rs in rasters:
            for r in rs:
                r._road_network = None  # what _reset does; reset() itself needs the entity in the scene at the first state
        ts, flags, frame_steps, poses = [], [], [], []
        maps = [[[] for _ in out["raster_cfg"]] for _ in obs]
        map_steps = [[] for _ in obs]
        step = 0
        while True:
            st = gym.state
            ts.append(st.t)
            flags.append([[d.step(st).future_collision for d in ds] for ds in detectors])
            if step % EVERY == 0:
                frame_steps.append(step)
                poses.append([st.poses[e] if e in st.poses else np.full(6, np.nan) for e in ents])
                for i, k in enumerate(obs):
                    if ents[k] in st.poses:
                        map_steps[i].append(step)
                        for c, r in enumerate(rasters[i]):
                            maps[i][c].append(np.asarray(r.step(st).map))
            if st.is_done:
                break
            gym.step()
            step += 1
        out[f"{n}/t"] = np.array(ts)
        out[f"{n}/future"] = np.array(flags, np.uint8)  # [steps + 1][observer][horizon]
        out[f"{n}/frame_steps"] = np.array(frame_steps, np.int64)
        out[f"{n}/poses"] = np.array(poses, np.float64)  # [frames][entity][6], NaN: not in state.poses
        for i, k in enumerate(obs):
            out[f"{n}/obs{i}/map_steps"] = np.array(map_steps[i], np.int64)
            for c, (w, h, m) in enumerate(out["raster_cfg"]):
                a = np.array(maps[i][c], np.uint8).reshape(len(map_steps[i]), len(LAYERS), int(m), int(m))
                out[f"{n}/obs{i}/map{c}"] = a  # [frames the observer is present in][layer][n][n]
        print(n, out[f"{n}/network"], "observers", obs, [ents[k].ref for k in obs], "steps", len(ts) - 1,
              "future", np.array(flags).sum(0).tolist(), "frames", [len(m) for m in map_steps],
              "ones", [[int(np.array(mm).sum()) for mm in m] for m in maps])
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(os.environ.get("SG_GOLDEN_OUT", HERE), "observers.npz"), **out)


if __name__ == "__main__":
    main()
