"""Time of one multi-agent tick of VectorScenarioEnv with device_tick=True (one sg_tick_drivers and the observation call, nothing
waited for) beside device_tick=False on the same batch -- sg_step_drivers, sg_terminal_flags, sg_entity_status_observers,
sg_route_observation_observers, reward and done in numpy, sg_reset_scenarios: the path the library had before and the yardstick.
A host clock around `step` and the engine's synchronize that follows it, device actions, driver_progress=1.0, warm, the two
environments interleaved in one process, median of 30 with min / max; then 100 device ticks queued back to back with one
synchronize at the end, per tick.
    python tools/driver_tick_time.py
4096 x 64 with 8 drivers per scenario, 256 x 16 with 2.  Writes profiles/driver_tick_time.json.
The environments are made from a synthetic packed batch, not from Scenario objects (a quarter of a million entities): the fields
`step` reads are filled in by hand, the engine calls are those of VectorScenarioEnv.__init__."""
import json
import os
import sys
import time

sys.path.insert(0, '.')
import numpy as np
import torch

import scenario_gym_amd as sga
import scenario_gym_amd._lib as L
from scenario_gym_amd import synthetic
from scenario_gym_amd.engine import terminal_mask
from scenario_gym_amd.road_network import LAYER_CODES

DT, N_PX, REPEATS, QUEUED = 0.1, 16, 30, 100
TERMS = ["max_length", "ego_collision"]  # (no road networks here: ego_off_road would end every episode at once)


def make_env(packed, per_scenario, device_tick):
    """A VectorScenarioEnv over `packed` whose slots 1..per_scenario of every scenario are the drivers (and the observers), each with
    its own recording as its route."""
    R, E = packed.n_scenarios, packed.n_entities
    env = object.__new__(sga.VectorScenarioEnv)
    env.scenarios, env.terminal_conditions, env.layers = [], TERMS, ["entity", "driveable_surface"]
    env._codes = [LAYER_CODES[l] for l in env.layers]
    env.height, env.width, env.n = 30.0, 30.0, N_PX
    env.auto_reset, env.torch_obs, env.driver_status, env.driver_progress, env.device_tick = True, True, True, 1.0, device_tick
    env._driver_obs, env._dev_bufs = [], {}  # (no driver_ttc, no driver_history)
    env.n_envs = R
    env._drv_env = np.repeat(np.arange(R, dtype=np.int32), per_scenario)
    env._drv_slot = np.tile(np.arange(1, per_scenario + 1, dtype=np.int32), R)
    env._trf_env = env._trf_slot = np.zeros(0, np.int32)
    env._ego = np.zeros(R, np.int64)
    env.engine = sga.RolloutEngine(R, E, timestep=DT, terminal_conditions=TERMS)
    env.engine.upload(packed)
    env.engine.set_road_networks([], np.full(R, -1, np.int32))
    env._lanes_set, env._routes_set, env._route_s0 = False, False, None
    env._mask = terminal_mask(TERMS)
    env.done = np.zeros(R, bool)
    env.engine.set_drivers(env._drv_env, env._drv_slot)
    env.engine.set_observers(env._drv_env, env._drv_slot)
    env._obs_env, env._obs_slot = env._drv_env, env._drv_slot
    g = env._drv_env.astype(np.int64) * E + env._drv_slot
    env.engine.set_routes(env._drv_env, env._drv_slot, [packed.knots[packed.knot_off[i]:packed.knot_off[i + 1], 1:3] for i in g])
    env._routes_set = True
    return env


def summary(x):
    x = np.asarray(x)
    return dict(median_us=float(np.median(x)), min_us=float(x.min()), max_us=float(x.max()), repeats=len(x))


def case(name, R, E, per_scenario):
    packed = synthetic.make_batch(R, E, n_steps=400, timestep=DT, n_knots=16, seed=5)
    kinds = packed.kind.reshape(R, E).copy()
    kinds[:, 1:per_scenario + 1] = L.KIND_AGENT_EXTERNAL
    packed.kind = kinds.ravel()
    host, dev = make_env(packed, per_scenario, False), make_env(packed, per_scenario, True)
    n = R * per_scenario
    rng = np.random.default_rng(3)
    acts = torch.as_tensor(np.stack([rng.uniform(-2, 2, n), rng.uniform(-0.3, 0.3, n)], -1), device="cuda:0").contiguous()
    host.reset()
    dev.reset()
    torch.cuda.synchronize()

    def tick(env):
        t0 = time.perf_counter()
        env.step(acts)
        env.engine.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for _ in range(5):
        tick(host)
        tick(dev)
    t_host, t_dev = [], []
    for _ in range(REPEATS):
        t_host.append(tick(host))
        t_dev.append(tick(dev))
    t_queued = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(QUEUED):
            dev.step(acts)
        dev.engine.synchronize()
        t_queued.append((time.perf_counter() - t0) * 1e6 / QUEUED)
    ratios = np.asarray(t_host) / np.asarray(t_dev)  # (pairs measured one after the other)
    out = dict(shape=[R, E], drivers=n, drivers_per_scenario=per_scenario, observation=[2, N_PX, N_PX], host_tick=summary(t_host),
               device_tick=summary(t_dev), device_tick_queued=dict(summary(t_queued), ticks_per_wait=QUEUED),
               host_over_device=float(np.median(t_host) / np.median(t_dev)), host_over_device_min=float(ratios.min()),
               host_over_device_max=float(ratios.max()), host_over_device_queued=float(np.median(t_host) / np.median(t_queued)),
               kernel=dev.engine.last_kernel())
    print(f"{name}: {R} x {E}, {n} drivers: device_tick=False median {out['host_tick']['median_us']:.0f} us (min {out['host_tick']['min_us']:.0f}, "
          f"max {out['host_tick']['max_us']:.0f}); device_tick=True median {out['device_tick']['median_us']:.0f} us (min "
          f"{out['device_tick']['min_us']:.0f}, max {out['device_tick']['max_us']:.0f}), ratio {out['host_over_device']:.2f} "
          f"({out['host_over_device_min']:.2f} .. {out['host_over_device_max']:.2f}); {QUEUED} queued: {out['device_tick_queued']['median_us']:.0f} us "
          f"per tick, ratio {out['host_over_device_queued']:.2f}")
    host.close()
    dev.close()
    return out


if __name__ == "__main__":
    res = dict(tool="tools/driver_tick_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0),
               large=case("4096 x 64, 8 drivers per scenario", 4096, 64, 8), small=case("256 x 16, 2 drivers per scenario", 256, 16, 2))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "driver_tick_time.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
