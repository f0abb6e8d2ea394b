#!/usr/bin/env python3
"""Golden vectors for several policy-driven vehicles in ONE scenario, from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_drivers.py   ->  tests/golden/drivers.npz

Two scenes of tests/driver_scenes.py (five entities: three of them agents with a VehicleController of their own, each fed its own
preset (accel, steer) sequence through the reference's plugin API, Agent._step -> VehicleAction; a static entity two of them run
into; one replayed entity) stepped through the reference's ScenarioGym at timestep 0.1 for 40 steps: per step the poses,
velocities and distances of State.  Only DATA is written."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path[:0] = [os.path.join(HERE, "_refstubs"), "/root/reference", os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import driver_scenes as DS  # noqa: E402
import scenario_gym  # noqa: E402
from scenario_gym import ScenarioGym  # noqa: E402
from scenario_gym.action import VehicleAction  # noqa: E402
from scenario_gym.agent import Agent, ReplayTrajectoryAgent  # noqa: E402
from scenario_gym.catalog_entry import BoundingBox, CatalogEntry  # noqa: E402
from scenario_gym.controller import VehicleController  # noqa: E402
from scenario_gym.entity import Entity  # noqa: E402
from scenario_gym.scenario import Scenario  # noqa: E402
from scenario_gym.sensor import EgoLocalizationSensor  # noqa: E402
from scenario_gym.trajectory import Trajectory  # noqa: E402

assert scenario_gym.__version__ == "0.3.1"
E = 5
# (no late spawn here: the reference's VehicleController._reset reads state.velocities[entity], which an entity that is not in the
# scene at the reset does not have)
CONFIG = [[(0, "a"), (2, "b"), (3, "free")], [(3, "a"), (0, "b"), (2, "free")]]


class PresetActionAgent(Agent):
    """Feeds a preset (accel, steer) sequence to the reference VehicleController (as make_golden.py's ExternalActionAgent)."""

    def __init__(self, entity, actions, **kw):
        super().__init__(entity, VehicleController(entity, **kw), EgoLocalizationSensor(entity))
        self.actions = actions
        self.k = 0

    def _reset(self):
        self.k = 0

    def _step(self, obs):
        a = self.actions[self.k]
        self.k += 1
        return VehicleAction(a[0], a[1])


def main():
    scs = DS.batch(E, CONFIG, seed=3)
    out = {"n": np.int64(len(scs)), "dt": np.float64(DS.DT), "steps": np.int64(DS.STEPS)}
    for i, sc in enumerate(scs):
        acts = DS.actions(len(sc["drivers"]), seed=100 + i)
        ents = []
        for e in range(E):
            ce = CatalogEntry(None, "e", "e", "Misc", BoundingBox(*sc["bbox"][e]), {}, [])
            ents.append(Entity(ce, trajectory=Trajectory(sc["knots"][sc["knot_off"][e]:sc["knot_off"][e + 1]]), ref="ego" if e == sc["ego"] else f"entity_{e}"))
        s = Scenario(ents, name=f"drivers_{i}")
        by_ref = {ents[slot].ref: j for j, slot in enumerate(sc["drivers"])}

        def create_agent(scenario, entity, sc=sc, acts=acts, by_ref=by_ref, ents=ents):
            if entity.ref in by_ref:
                j = by_ref[entity.ref]
                c = sc["ctrl"][sc["drivers"][j]]
                return PresetActionAgent(entity, acts[:, j], max_steer=float(c[0]), max_accel=float(c[1]),
                                         max_speed=None if np.isnan(c[2]) else float(c[2]), allow_reverse=bool(c[3]))
            if entity.ref == "ego":
                return ReplayTrajectoryAgent(entity)

        gym = ScenarioGym(timestep=DS.DT, terminal_conditions=[])
        gym.set_scenario(s, create_agent=create_agent)
        st = gym.state
        ents = s.entities
        off = [0]
        for e in ents:
            off.append(off[-1] + e.trajectory.data.shape[0])
        P, V, D, T = [], [], [], []

        def snap():
            T.append(st.t)
            P.append([st.poses[e] if e in st.poses else np.full(6, np.nan) for e in ents])
            V.append([st.velocities[e] if e in st.velocities else np.full(6, np.nan) for e in ents])
            D.append([st.distances[e] for e in ents])

        snap()
        for _ in range(DS.STEPS):
            gym.step()
            snap()
        p = f"{i}/"
        out.update({
            p + "scenario/knot_off": np.array(off, np.int64), p + "scenario/knots": np.concatenate([e.trajectory.data for e in ents]),
            p + "scenario/bbox": np.asarray(sc["bbox"], np.float64), p + "scenario/etype": np.full(E, 2, np.int32),
            p + "scenario/refs": np.array([e.ref for e in ents]), p + "scenario/ego": np.int64(ents.index(s.ego)),
            p + "scenario/length": np.float64(s.length), p + "drivers": np.array(sc["drivers"], np.int64),
            p + "ctrl": sc["ctrl"][sc["drivers"]][:, :4], p + "actions": acts,
            p + "t": np.array(T), p + "poses": np.array(P, np.float64), p + "vels": np.array(V, np.float64), p + "dists": np.array(D, np.float64),
        })
        print(i, "steps", len(T) - 1, "present at reset", int((~np.isnan(np.array(P)[0, :, 0])).sum()), "at the end", int((~np.isnan(np.array(P)[-1, :, 0])).sum()))
    np.savez_compressed(os.path.join(os.environ.get("SG_GOLDEN_OUT", HERE), "drivers.npz"), **out)


if __name__ == "__main__":
    main()
