#!/usr/bin/env python3
"""Golden vectors for the replay interpolant on per-entity knot times, from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_knots.py      -> tests/golden/knots.npz

Small editions (8 entities -- `long`: 6 of 128 .. 256 knots --, 24 steps) of every family of tests/knot_scenes.py: knots ON the
clock's values and one ulp beside them, knots one ulp apart, a union grid of a thousand rows, a clock from 0.37.  Per family
and timestep (`<family>/dt10`: scenario 0 at dt = 0.1; `<family>/dt30`: scenario 1, which carries z / pitch / roll, at 1/30):

  scenario            the entities as the reference's Trajectory constructor left them (export_scenario)
  replay_nopersist    ScenarioGym rollouts as make_golden.record_rollout records them (pose, velocity, distance, collisions
  replay_persist      of every entity after every step, metrics, events): the default agents, persist off and on,
  pid                 and the ego driven by the reference's PIDAgent (+ its controller state after every step)
  batch_nopersist     BatchReplayEntity.step itself, ALL entities batched, at the clock's times (State.next_t of every step):
  batch_persist       poses [steps + 1][E][6], NaN = not returned

Only data is written (the generator's numbers and the reference's outputs); tests/test_knot_times_cpu.py reads it.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import make_golden as G  # noqa: E402  (sets up the import stand-ins and imports the reference)
from scenario_gym import ScenarioGym  # noqa: E402
from scenario_gym.agent import PIDAgent  # noqa: E402
from scenario_gym.entity.batch import BatchReplayEntity  # noqa: E402
from scenario_gym.scenario import Scenario  # noqa: E402

import knot_scenes as KS  # noqa: E402  (the build's own scene generator: numbers only)

STEPS = 24
RUNS = (("dt10", 0.1, 0), ("dt30", 1.0 / 30.0, 1))  # (name, timestep, scenario of the family)


def small(family, dt, r):
    return KS.scene(family, 6 if family == "long" else 8, r, "replay", dt, STEPS, K=24)


def entities(sc):
    off = sc["knot_off"]
    return [G.make_entity(sc["knots"][off[e]:off[e + 1]], "ego" if e == 0 else f"entity_{e}", bbox=tuple(sc["bbox"][e]))
            for e in range(len(off) - 1)]


def batch_step(ents, q, persist):
    class FakeState:
        next_t = 0.0

    b = BatchReplayEntity(persist=persist)
    b.add_entities(ents, [e.trajectory for e in ents])
    P = np.full((len(q), len(ents), 6), np.nan)
    for i, t in enumerate(q):
        FakeState.next_t = float(t)
        for e, p in b.step(FakeState).items():
            P[i, ents.index(e)] = p
    return P


def pid_agent(sc, e):
    if e.ref == "ego":
        return PIDAgent(e)


def pid_extra(g):
    c = g.state.agents[g.state.scenario.ego].controller
    return [c.speed, c.e_lon_prev, c.e_lat_prev, c.e_lon_int]


def main():
    out = {}
    for family in KS.FAMILIES:
        for name, dt, r in RUNS:
            key = f"{family}/{name}"
            sc = small(family, dt, r)
            ents = entities(sc)
            s = Scenario(ents, name=f"knots_{family}_{name}")
            exp = G.export_scenario(s)
            del exp["refs"]
            out.update(G.flat(key + "/scenario", exp))
            out[key + "/generated_knots_equal"] = np.bool_(np.array_equal(exp["knots"], sc["knots"]))
            for pname, persist in (("nopersist", False), ("persist", True)):
                gym = ScenarioGym(timestep=dt, persist=persist, metrics=G.std_metrics())
                gym.set_scenario(s)
                out.update(G.flat(f"{key}/replay_{pname}", G.record_rollout(gym, max_steps=STEPS)))
                out[f"{key}/batch_{pname}"] = batch_step(ents, KS.clock(sc["t0"], dt, STEPS), persist)
            gym = ScenarioGym(timestep=dt, metrics=G.std_metrics())
            gym.set_scenario(s, create_agent=pid_agent)
            out.update(G.flat(f"{key}/pid", G.record_rollout(gym, max_steps=STEPS, extra=pid_extra)))
            print(key, int(out[f"{key}/replay_nopersist/n_steps"]), "steps,", len(out[f"{key}/replay_nopersist/ev_t"]), "events", flush=True)
    path = os.path.join(os.environ.get("SG_GOLDEN_OUT", HERE), "knots.npz")
    np.savez_compressed(path, **out)
    print(f"knots: {len(out)} arrays, {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
