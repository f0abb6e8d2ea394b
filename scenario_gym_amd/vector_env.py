"""A vector of scenario_gym RL environments on one device.

The reference's `integrations/openaigym.py` wraps ONE ScenarioGym as a gym `Env`: `step(action)` runs the ego's
VehicleController with the policy's (acceleration, steering), every other entity by its trajectory, then returns the
ego's rasterized-map observation, the agent's reward and `state.is_done` (:171-226); the defaults are
terminal_conditions ["max_length", "ego_collision", "ego_off_road"] (:93-94), `VehicleController(max_steer=0.9,
max_accel=5.0)` and `MapOnlySensor(channels_first=True, height=30, width=30, n=128)` with the default layers
(entity, driveable_surface) (:280-293), reward -1 for a done state that is off the road or in an ego collision and 0.01
otherwise (:300-310).  `VectorScenarioEnv` is that loop for R scenarios at once: one `sg_tick` per tick (the step with the
[R, 2] actions, the terminal conditions and the map observation replayed as one captured hipGraph) and
`sg_reset_scenarios` for the environments whose episode ended.  No arithmetic of the environment runs on the host.

`drivers=`: several policy-driven vehicles per environment (the reference accepts any number of agents with a
VehicleController in one scenario).  Every listed entity is a driver of the engine (`sg_set_drivers`); a tick is
`sg_step_drivers` with one (acceleration, steering) per driver, then `sg_terminal_flags`; the observations are those of the
observer list, which the drivers form by default.

`traffic=`: background traffic that reacts.  Every listed entity is run by the engine's built-in policy (IDM car-following)
along its own recorded trajectory (`sg_set_driver_policy`): a driver appended behind the caller's drivers, whose actions the
device makes itself.  A tick is then one `sg_step_drivers_policy`; `step` keeps taking the caller's drivers' actions alone.

With a driver list the reward, the done flags, the progress and the auto-reset of a tick are numpy on the host between synchronous
calls -- unless `device_tick=True` (with torch_obs): then a tick is one `sg_tick_drivers`, which does all of that on the device in
stream order, and the observation call queued behind it; actions, rewards, dones and info are tensors in HBM and the host waits for
nothing.
"""
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from .agent import ExternalVehicleAgent, ReplayTrajectoryAgent
from .engine import RolloutEngine, terminal_mask
from .obs_table import KINDS, public_call
from .packing import pack_scenarios
from .road_network import LAYER_CODES, shared_lane_arrays, shared_polygon_arrays
from .scenario import Scenario


class EnvState:
    """What VectorScenarioEnv.save_state returns: the engine's Snapshot and the environment's host state beside it."""

    def __init__(self, snapshot, done, route_s0):
        self.snapshot, self.done, self.route_s0 = snapshot, done, route_s0

    def close(self):
        self.snapshot.close()


class VectorScenarioEnv:
    def __init__(self, scenarios: Sequence[Scenario], timestep: float = 0.1,
                 terminal_conditions: Optional[Sequence[str]] = None, layers: Optional[Sequence[str]] = None,
                 height: float = 30.0, width: float = 30.0, n: int = 128, max_steer: float = 0.9, max_accel: float = 5.0,
                 auto_reset: bool = True, torch_obs: bool = False, device: int = 0,
                 drivers: Optional[Sequence[Sequence[int]]] = None, driver_status: bool = True,
                 traffic: Optional[Sequence[Sequence[int]]] = None, traffic_params=None,
                 driver_progress: Optional[float] = None, device_tick: bool = False, driver_ttc: Optional[float] = None,
                 driver_history: Optional[dict] = None):
        """drivers: per environment the entity indices (positions in scenarios[i].entities) the policy drives, each with a
        VehicleController(max_steer, max_accel); None: the ego of every environment, one action per environment.
        driver_status: with a driver list, every step also reports the episode status of every driver (sg_entity_status_observers)
        and a reward and a done flag per driver in `info`; False: nothing is added and nothing is launched.
        traffic: per environment the entity indices the engine's built-in policy runs along their own recorded trajectory
        (trajectory.data[:, 1:3] as given), each with the same VehicleController; needs `drivers`, and no entity may be in both.
        traffic_params: None, keyword arguments of idm_params for every traffic entity (a dict), or one parameter row per traffic
        entity ([n_traffic, DP_NPARAM], environment by environment); v0 defaults to the largest knot-to-knot speed of the
        entity's recording, floored at 1 m/s.  {"corridor": "path"} makes the traffic look for its lead in a corridor bent along
        its recorded trajectory, so it follows a lead round a bend; the default is the straight corridor in its heading frame.
        driver_progress: None, or the weight w of a progress term in the per-driver reward (needs `drivers` and driver_status):
        every driver gets a route -- its own recorded trajectory unless set_routes gave another -- and every step reports in
        `info` driver_route (the rows of sg_route_observation_observers) and driver_progress (the arclength gained along the
        route since the previous tick; 0 for a driver without a route, not in the scene at either tick, or when reset() or an
        auto-reset of its environment came in between), and adds w * driver_progress to driver_reward.
        device_tick: with `drivers` and torch_obs, a tick is ONE sg_tick_drivers -- step, terminal conditions, driver status and
        route rows, reward, done, progress, episode statistics and the auto-reset, all on the device in stream order -- and the
        observation call behind it.  `step` takes a float64 tensor [n_drivers, 2] on the device and returns torch tensors in HBM
        alone, ordered on torch's current stream; nothing is copied to the host and nothing waits for the device.  The values are
        those of the default path, bit for bit; `info` also carries episode_return [n_drivers] and episode_length [R] (of the
        episode up to and including this tick).  The tensors are views of buffers the engine owns: the next step overwrites
        them.  No `done` bookkeeping is kept on the host: auto_reset=False never resets and never raises -- a finished environment
        simply goes on stepping, and the caller decides (reset(), engine.reset_scenarios_device).
        driver_ttc: None, or the horizon H in seconds (inf: unbounded) of a time-to-collision row per driver (needs `drivers`):
        every step reports in `info` driver_ttc [n_drivers, 4] and driver_ttc_info [n_drivers, 3], the rows of
        sg_time_to_collision_observers for the drivers on the state the returned `obs` describes -- after an auto-reset, unlike
        driver_flags -- and reset() leaves the same two in `reset_info`.  numpy arrays, or with torch_obs tensors in HBM; with
        device_tick the call is queued behind the tick and nothing crosses PCIe (an observer list of the caller's own that differs
        from the driver list is swapped around the call, and each swap waits for the stream).  Not part of driver_reward.
        driver_history: None, or dict(samples=H, stride=s, k=k, radius=r) (stride 1, k 0 and radius inf unless given) for a pose
        history per driver (needs `drivers`, and "max_length" among the terminal conditions, which bounds an episode): every
        reset() and step() reports driver_history [n_drivers, 1 + k, H, 6], driver_history_slots [n_drivers, k] and
        driver_history_count [n_drivers], the rows of sg_pose_history_observers for the drivers -- where each driver and its k
        nearest entities were at the last H ticks, s ticks apart, in the driver's current frame -- on the state the returned
        `obs` describes, behind an auto-reset as driver_ttc is: a new episode starts with one valid sample.  Delivered and
        queued as driver_ttc is.  The engine then keeps a pose record of the longest episode of the batch, rows = the steps at
        which max_length ends it + the reset row (+ one step of slack for the rounding of the clock), which costs rows * 6 * R *
        EP * 8 bytes of device memory (EP: the entities per environment rounded up to 64) and is copied by save_state.  (A
        ring-shaped record would cut that to H * s rows, but it would change every stepping kernel.)  An environment that goes
        on stepping past its end (device_tick with auto_reset=False) overruns the record: its rows are zero and its count -2
        until it is reset.  Not part of driver_reward."""
        self.scenarios = list(scenarios)
        self.terminal_conditions = list(terminal_conditions) if terminal_conditions is not None else \
            ["max_length", "ego_collision", "ego_off_road"]
        self.layers = list(layers) if layers is not None else ["entity", "driveable_surface"]
        self._codes = [LAYER_CODES[l] for l in self.layers]
        self.height, self.width, self.n = float(height), float(width), int(n)
        self.auto_reset, self.torch_obs = auto_reset, torch_obs
        self.driver_status = bool(driver_status)
        self.driver_progress = None if driver_progress is None else float(driver_progress)
        if self.driver_progress is not None and (drivers is None or not self.driver_status):
            raise ValueError("driver_progress: needs a driver list (drivers=...) with driver_status")

        self.driver_ttc = None if driver_ttc is None else float(driver_ttc)
        if self.driver_ttc is not None and drivers is None:
            raise ValueError("driver_ttc: needs a driver list (drivers=...)")
        self.driver_history = None
        if driver_history is not None:
            if drivers is None:
                raise ValueError("driver_history: needs a driver list (drivers=...)")
            if "max_length" not in self.terminal_conditions:
                raise ValueError('driver_history: needs "max_length" among the terminal conditions (it bounds the pose record)')
            unknown = set(driver_history) - {"samples", "stride", "k", "radius"}
            if unknown or "samples" not in driver_history:
                raise ValueError("driver_history: dict(samples=H, stride=1, k=0, radius=inf)")
            self.driver_history = (int(driver_history["samples"]), int(driver_history.get("stride", 1)), int(driver_history.get("k", 0)),
                                   float(driver_history.get("radius", float("inf"))))
        # the configured driver observations: (kind, arguments, those its *_observers_queued form takes behind the tensors, the
        # `info` keys of its outputs); the tensors device_tick queues them into, by kind
        self._driver_obs, self._dev_bufs = [], {}
        if self.driver_ttc is not None:
            self._driver_obs.append(("ttc", (self.driver_ttc,), (self.driver_ttc,), ("driver_ttc", "driver_ttc_info")))
        if self.driver_history is not None:
            self._driver_obs.append(("pose_history", self.driver_history, self.driver_history[1::2],  # (stride, radius: the tensors tell the rest)
                                     ("driver_history", "driver_history_slots", "driver_history_count")))
        self.reset_info = {}
        self.device_tick = bool(device_tick)
        if self.device_tick and (drivers is None or not torch_obs):
            raise ValueError("device_tick: needs a driver list (drivers=...) and torch_obs=True")
        if self.device_tick and self.driver_progress == 0.0:
            raise ValueError("device_tick: driver_progress=0 launches no route observation; pass None to switch the term off")

        if drivers is not None and len(drivers) != len(self.scenarios):
            raise ValueError("drivers: one list of entity indices per environment")
        if traffic is not None:
            if drivers is None:
                raise ValueError("traffic: needs a driver list (drivers=...)")
            if len(traffic) != len(self.scenarios):
                raise ValueError("traffic: one list of entity indices per environment")
            for i, (ds, ts) in enumerate(zip(drivers, traffic)):
                both = {int(k) for k in ds} & {int(k) for k in ts}
                if both:
                    raise ValueError(f"traffic: entities {sorted(both)} of environment {i} are listed as drivers too")

        def create_agent(scenario, entity):  # openaigym.py:280-293: the ego is driven by the policy
            if entity is scenario.ego:
                if drivers is None:
                    return ExternalVehicleAgent(entity, max_steer=max_steer, max_accel=max_accel)
                return ReplayTrajectoryAgent(entity)  # (unless it is listed, below: the reference's default agent)

        packed, _ = pack_scenarios(self.scenarios, create_agent)
        self._drv_env = self._drv_slot = None
        self._trf_env = self._trf_slot = np.zeros(0, np.int32)
        if drivers is not None:
            # the driven slots: caller-run slots whose VehicleController the device steps itself (sg_set_drivers)
            self._drv_env = np.array([i for i, ks in enumerate(drivers) for _ in ks], np.int32)
            self._drv_slot = np.array([int(k) for ks in drivers for k in ks], np.int32)
            # ... and behind them the traffic, whose actions the built-in policy makes (sg_set_driver_policy)
            self._trf_env = np.array([i for i, ks in enumerate(traffic or []) for _ in ks], np.int32)
            self._trf_slot = np.array([int(k) for ks in (traffic or []) for k in ks], np.int32)
            for i, k in zip(np.concatenate([self._drv_env, self._trf_env]), np.concatenate([self._drv_slot, self._trf_slot])):
                agent = ExternalVehicleAgent(self.scenarios[i].entities[k], max_steer=max_steer, max_accel=max_accel)
                packed.kind[int(i) * packed.n_entities + int(k)] = L.KIND_AGENT_EXTERNAL
                packed.ctrl[int(i) * packed.n_entities + int(k)] = agent.controller.ctrl_row()
        self.n_envs = packed.n_scenarios
        self._ego = np.array([sc.entities.index(sc.ego) for sc in self.scenarios], np.int64)
        record_rows = 0
        if self.driver_history is not None:
            # max_length ends an episode behind the first step n >= 1 with t0 + n * dt + dt > length (check_terminal on the
            # device): n = max(1, floor((length - t0) / dt)); one more for the rounding of the summed clock, one for the reset row
            longest = float(np.max(np.asarray(packed.length, np.float64) - np.asarray(packed.t0, np.float64)))
            record_rows = max(1, int(np.floor(max(longest, 0.0) / float(timestep)))) + 2
        self.engine = RolloutEngine(packed.n_scenarios, packed.n_entities, timestep=timestep,
                                    terminal_conditions=self.terminal_conditions, device=device, record_capacity=record_rows)
        self.engine.upload(packed)
        self.engine.set_road_networks(*shared_polygon_arrays(self.scenarios))
        self._lanes_set = False  # the lane centre lines go down when a lane observation is first asked for
        self._mask = terminal_mask(self.terminal_conditions)
        self.done = np.zeros(self.n_envs, bool)
        self._obs_env, self._obs_slot = np.zeros(0, np.int32), np.zeros(0, np.int32)  # set_observers
        if drivers is not None:
            self.engine.set_drivers(np.concatenate([self._drv_env, self._trf_env]), np.concatenate([self._drv_slot, self._trf_slot]))
            self.set_observers(drivers)  # (the default: every driver of the caller's observes)
            if self.n_traffic:
                self._set_traffic_policy(traffic_params)
        self._routes_set = False     # the routes go down when a route observation is first asked for
        self._route_s0 = None        # driver_progress: (arclength, on a route) of every driver at the previous tick
        if self.driver_progress is not None:
            self.set_routes()

    def _set_traffic_policy(self, traffic_params):
        """The policy rows and paths of the traffic entities: each along its own recorded trajectory."""
        from .engine import idm_params

        paths, rows = [], []
        for i, k in zip(self._trf_env, self._trf_slot):
            data = np.asarray(self.scenarios[i].entities[k].trajectory.data, np.float64)
            paths.append(data[:, 1:3])
            dt = np.diff(data[:, 0])
            speed = np.hypot(np.diff(data[:, 1]), np.diff(data[:, 2]))[dt > 0] / dt[dt > 0]
            kw = dict(v0=max(1.0, float(speed.max()) if len(speed) else 0.0))
            if isinstance(traffic_params, dict):
                kw.update(traffic_params)
            rows.append(idm_params(**kw))
        if traffic_params is not None and not isinstance(traffic_params, dict):
            rows = np.asarray(traffic_params, np.float64).reshape(self.n_traffic, L.DP_NPARAM)
        self.engine.set_driver_policy(self.n_drivers + np.arange(self.n_traffic), np.array(rows), paths)

    @property
    def n_drivers(self):
        """The caller's drivers (the traffic is not counted: its actions are the engine's)."""
        return 0 if self._drv_env is None else len(self._drv_env)

    @property
    def n_traffic(self):
        """The entities the built-in policy runs (`traffic=`)."""
        return len(self._trf_env)

    @property
    def observation_shape(self):
        return (len(self.layers), self.n, self.n)  # channels first, as MapOnlySensor(channels_first=True)

    def _observe(self):
        if self._drv_env is not None:  # the observations of the observer list (the drivers, unless set_observers changed it)
            return self.observe_entities()[0]
        if self.torch_obs:
            return self.engine.raster_map_torch(self._codes, self.width, self.height, self.n, self.n)
        return self.engine.raster_map(self._codes, self.width, self.height, self.n, self.n)

    def reset(self):
        """Env.reset for every environment (openaigym.py:128-169): observations [R, n_layers, n, n]."""
        self.engine.reset()
        self.done[:] = False
        self._route_s0 = None
        self.reset_info = self._driver_obs_info()
        return self._observe()

    def save_state(self):
        """A token of the state of every environment as it is now: an engine Snapshot (sg_snapshot_create: allocates, may wait
        for the device) and the environment's own per-episode host state, `done` and the previous arclengths of the progress
        reward.  With device_tick there is no host state.  restore_state(token) goes back to it any number of times;
        token.close() frees it (close() of the environment does too)."""
        route = None if self._route_s0 is None else (self._route_s0[0].copy(), self._route_s0[1].copy())
        return EnvState(self.engine.snapshot(), None if self.device_tick else self.done.copy(), route)

    def restore_state(self, token, mask=None):
        """Back to the state of save_state for every environment, or for those with mask[i] != 0 (numpy bool / uint8 [R], or with
        device_tick a torch uint8 / bool tensor on the device, read in stream order): the engine's state (sg_snapshot_restore,
        queued, not waited for), and on the default path `done` and the previous arclengths of the masked environments and their
        drivers, nobody else's.  Every later step returns for them what it would have returned right after save_state.  Returns
        the observation of the restored state as reset() returns it, and leaves reset_info as reset() does."""
        token.snapshot.restore(mask)
        if not self.device_tick:
            m = np.ones(self.n_envs, bool) if mask is None else np.asarray(mask).astype(bool)
            self.done[m] = token.done[m]
            if self._drv_env is not None and (token.route_s0 is not None or self._route_s0 is not None):
                md = m[self._drv_env]
                if self._route_s0 is None:
                    self._route_s0 = (np.zeros(self.n_drivers), np.zeros(self.n_drivers, bool))
                saved = token.route_s0 if token.route_s0 is not None else (np.zeros(self.n_drivers), np.zeros(self.n_drivers, bool))
                self._route_s0[0][md] = saved[0][md]
                self._route_s0[1][md] = saved[1][md]
        self.reset_info = self._driver_obs_info()
        return self._observe()

    def step(self, actions):
        """actions [R, 2] = (acceleration, steering) per environment (numpy, or a float64 torch tensor on the device).
        Returns (obs, reward [R], done [R], info).  With auto_reset the environments that finished are reset and their
        observation is the first of the new episode; without it, stepping a finished environment raises as the reference's
        `step` does."""
        if self.device_tick:
            return self._step_device(actions)
        if not self.auto_reset and self.done.any():
            raise ValueError("Step called when state is terminal.")
        if self._drv_env is not None:
            return self._step_drivers(actions)
        if not hasattr(actions, "data_ptr"):
            actions = np.asarray(actions, np.float64).reshape(self.n_envs, 2)
        # step + terminal conditions + observation: one captured graph launch (sg_tick)
        obs, flags = self.engine.tick(actions, self._codes, self.width, self.height, self.n, self.n, torch_out=self.torch_obs)
        if self.torch_obs:
            flags = flags.cpu().numpy().astype(np.uint32)
        done, reward = self._done_reward(flags)
        self.done = done
        if self.auto_reset and done.any():
            self.engine.reset_scenarios(done)
            self.done = np.zeros(self.n_envs, bool)
            obs = self._observe()  # the restarted environments return the first observation of their new episode
        return obs, reward, done, {"terminal_flags": flags}

    def _done_reward(self, flags):
        """(done [R], reward [R]) of the terminal flags of a tick: the engine's terminal conditions; RLAgent.reward
        (openaigym.py:300-310), -1 for a done state that is off the road or in an ego collision and 0.01 otherwise."""
        done = (flags & self._mask) != 0
        bad = (flags & (L.TERM_EGO_OFF_ROAD | L.TERM_EGO_COLLISION)) != 0
        return done, np.where(done & bad, -1.0, 0.01)

    def _step_drivers(self, actions):
        """step() with a driver list: actions [n_drivers, 2] in list order (environment by environment, each in the order of
        its `drivers` entry).  sg_step_drivers (with traffic: sg_step_drivers_policy), then sg_terminal_flags; reward, done and auto-reset per environment as without
        drivers; with driver_status, info also holds driver_flags [n_drivers], driver_info [n_drivers, 4], driver_feat
        [n_drivers, 3] (sg_entity_status_observers on the stepped state, before an auto-reset), driver_reward [n_drivers] (-1 for
        a driver that is off the road or in a collision, else 0.01) and driver_done [n_drivers] (that, or its environment
        done); with driver_progress=w also driver_route [n_drivers, 11] (sg_route_observation_observers on the stepped state) and
        driver_progress [n_drivers], and driver_reward has w * driver_progress added; obs [n_observers, n_layers, n, n] of the
        observer list (observe_entities)."""
        if not hasattr(actions, "data_ptr"):
            actions = np.asarray(actions, np.float64).reshape(self.n_drivers, 2)
        if self.n_traffic:
            # the traffic's rows follow the caller's; the policy fills them on the device (one sg_step_drivers_policy per tick)
            if hasattr(actions, "data_ptr"):
                import torch

                full = torch.cat([actions.reshape(self.n_drivers, 2), actions.new_zeros((self.n_traffic, 2))]).contiguous()
            else:
                full = np.concatenate([actions, np.zeros((self.n_traffic, 2))])
            self.engine.step_drivers_policy(full, 1)
        else:
            self.engine.step_drivers(actions, 1)
        flags = self.engine.terminal_flags()
        done, reward = self._done_reward(flags)
        info = {"terminal_flags": flags}
        if self.driver_status and self.n_drivers:  # the stepped state, before an auto-reset replaces it
            d_flags, d_info, d_feat = self._driver_status()
            d_bad = (d_flags & (L.ST_OFF_ROAD | L.ST_COLLISION)) != 0
            info.update(driver_flags=d_flags, driver_info=d_info, driver_feat=d_feat,
                        driver_reward=np.where(d_bad, -1.0, 0.01),  # RLAgent.reward asked per driver, without its is_done gate
                        driver_done=d_bad | done[self._drv_env])
            if self.driver_progress is not None:
                if self._route_s0 is None:  # (the first tick of the run: the arclengths of the reset state were not asked for)
                    self._route_s0 = (np.zeros(self.n_drivers), np.zeros(self.n_drivers, bool))
                feat, r_info = self._driver_call(lambda: self.engine.route_observation(0, 0.0, observers=True))
                on = r_info[:, 0] >= 0  # (on a route, which says in the scene too)
                progress = np.where(on & self._route_s0[1], feat[:, 8] - self._route_s0[0], 0.0)
                info.update(driver_route=feat, driver_progress=progress)
                info["driver_reward"] = info["driver_reward"] + self.driver_progress * progress
                self._route_s0 = (feat[:, 8].copy(), on)
        self.done = done
        if self.auto_reset and done.any():
            self.engine.reset_scenarios(done)  # (the reset restarts the drivers' controller speeds with the rest of the state)
            self.done = np.zeros(self.n_envs, bool)
            if self._route_s0 is not None:  # a new episode: its first tick has no previous arclength
                self._route_s0[1][done[self._drv_env]] = False
        info.update(self._driver_obs_info())  # (the state the observation describes: behind the auto-reset)
        return self._observe(), reward, done, info

    def _step_device(self, actions):
        """step() with device_tick: one sg_tick_drivers and the observation call, no host round trip (see __init__)."""
        import torch

        nd, nt = self.n_drivers, self.n_traffic
        actions = actions.reshape(nd, 2)
        if nt:  # the traffic's rows follow the caller's; the policy fills them on the device
            if getattr(self, "_dev_actions", None) is None:
                self._dev_actions = actions.new_zeros((nd + nt, 2))
            self._dev_actions[:nd].copy_(actions)
            actions = self._dev_actions
        shape = (len(self._obs_env),) + self.observation_shape
        if getattr(self, "_dev_obs", None) is None or tuple(self._dev_obs.shape) != shape:
            self._dev_obs = torch.empty(shape, dtype=torch.uint8, device=actions.device)
        with self.engine.ordered_with_torch():  # the tick and the observation behind the policy's writes, as one
            v = self.engine.tick_drivers(actions.contiguous(), terminal_mask=self._mask, auto_reset=self.auto_reset,
                                         w_progress=self.driver_progress or 0.0, ordered=False)
            obs = self.engine.raster_map_observers_queued(self._dev_obs, self._codes, self.width, self.height, self.n, self.n, ordered=False)
            ttc = self._driver_obs_info(queued=True)
        info = {"terminal_flags": v["term_flags"], "episode_return": v["ep_return"][:nd], "episode_length": v["ep_length"], **ttc}
        if self.driver_status and nd:
            info.update(driver_flags=v["drv_flags"][:nd], driver_info=v["drv_info"][:nd], driver_feat=v["drv_feat"][:nd],
                        driver_reward=v["drv_reward"][:nd], driver_done=v["drv_done"][:nd].view(torch.bool))
            if self.driver_progress is not None:
                info.update(driver_route=v["drv_route"][:nd], driver_progress=v["drv_progress"][:nd])
        return obs, v["env_reward"], v["env_done"].view(torch.bool), info

    def _driver_obs_info(self, queued=False):
        """The `info` entries of the configured driver observations (driver_ttc=H: driver_ttc [n_drivers, 4], driver_ttc_info
        [n_drivers, 3], sg_time_to_collision_observers; driver_history=dict(...): driver_history [n_drivers, 1 + k, H, 6],
        driver_history_slots [n_drivers, k], driver_history_count [n_drivers], sg_pose_history_observers) of the drivers at the
        current state, in that order; {} without any.  queued (device_tick, inside its ordered_with_torch block): into tensors
        the environment keeps, on the engine's stream with no host wait."""
        out = {}
        for kind, args, queued_args, keys in self._driver_obs if self.n_drivers else ():
            if queued:
                bufs = self._dev_bufs.get(kind)
                if bufs is None:
                    import torch

                    specs = KINDS[kind].outs(self.n_drivers, *KINDS[kind].args(*args)[0])
                    bufs = self._dev_bufs[kind] = tuple(torch.empty(shape, dtype=getattr(torch, dt), device=self._dev_obs.device)
                                                        for shape, _, dt in specs)
                call = lambda: getattr(self.engine, KINDS[kind].observers + "_queued")(*bufs, *queued_args, ordered=False)  # noqa: E731
            else:
                call = lambda: public_call(self.engine, kind, True, args, torch_out=self.torch_obs)  # noqa: E731
            out.update(zip(keys, self._driver_call(call)))
        return out

    def _driver_status(self):
        """(flags [n_drivers], info [n_drivers, 4], feat [n_drivers, 3]) of the drivers at the current state, as numpy arrays."""
        return self._driver_call(self.engine.entity_status_observers)

    def _driver_call(self, call):
        """call() with the drivers as the engine's observers: through the observer list when that is the driver list (the
        default); otherwise the drivers are the engine's observers for this one call and the caller's list is put back."""
        same = np.array_equal(self._obs_env, self._drv_env) and np.array_equal(self._obs_slot, self._drv_slot)
        if not same:
            self.engine.set_observers(self._drv_env, self._drv_slot)
        try:
            return call()
        finally:
            if not same:
                self.engine.set_observers(self._obs_env, self._obs_slot)

    def _observation(self, kind, observers, *args):
        """Observation `kind` (a row of obs_table.KINDS) of the egos, or of the observers of set_observers with (env_of_observer
        [n], slot [n]) behind its outputs; what the row needs on the device goes down first.  torch_obs: torch tensors in HBM."""
        if "lanes" in KINDS[kind].needs:
            self._set_lanes()
        if "routes" in KINDS[kind].needs and not self._routes_set:
            self.set_routes()
        out = public_call(self.engine, kind, observers, args, torch_out=self.torch_obs)
        return tuple(out) + self._observer_index(out[0]) if observers else out

    def status(self):
        """The episode status of the ego of every environment at the current state (sg_entity_status): (flags [R] ST_* bits, info
        [R, 4], feat [R, 3]: RolloutEngine.entity_status).  torch_obs: torch tensors in HBM; else numpy arrays."""
        return self._observation("entity_status", False)

    def observe_entities_status(self):
        """The episode status of every observer of set_observers at the current state (sg_entity_status_observers): (flags [n],
        info [n, 4], feat [n, 3], env_of_observer [n], slot [n]).  torch_obs: torch tensors in HBM; else numpy arrays."""
        return self._observation("entity_status", True)

    def time_to_collision(self, horizon: float = float("inf")):
        """The time to collision of the ego of every environment at the current state (sg_time_to_collision): (feat [R, 4], info
        [R, 3]: RolloutEngine.time_to_collision).  torch_obs: torch tensors in HBM; else numpy arrays."""
        return self._observation("ttc", False, horizon)

    def time_to_collision_observers(self, horizon: float = float("inf")):
        """The time to collision of every observer of set_observers at the current state (sg_time_to_collision_observers): (feat
        [n, 4], info [n, 3], env_of_observer [n], slot [n]).  torch_obs: torch tensors in HBM; else numpy arrays."""
        return self._observation("ttc", True, horizon)

    def road_info(self, cap: int = 32):
        """State.get_road_info_at_entity for the ego of every environment (sg_road_info): count [R], geoms [R, cap] indices
        into the scenario's `road_network.geometry_index()`, layers [R] LAYER_* bits.  torch_obs: torch tensors in HBM (lists
        stop at cap); else numpy arrays (no list truncated)."""
        count, geoms, layers = self.engine.road_info(cap, torch_out=self.torch_obs)
        if self.torch_obs:
            import torch

            r = torch.arange(self.n_envs, device=count.device)
            e = torch.as_tensor(self._ego, device=count.device)
            return count[r, e], geoms[r, e], layers[r, e]
        r = np.arange(self.n_envs)
        return count[r, self._ego], geoms[r, self._ego], layers[r, self._ego]

    def set_observers(self, slots):
        """Entities other than (or beside) the ego that observe_entities() reports for: slots[i] = the entity indices
        (positions in scenarios[i].entities) of environment i.  Replaces the previous list; all lists empty clears it."""
        if len(slots) != self.n_envs:
            raise ValueError("set_observers: one list of entity indices per environment")
        env = [i for i, ks in enumerate(slots) for _ in ks]
        slot = [int(k) for ks in slots for k in ks]
        self.engine.set_observers(env, slot)
        self._obs_env, self._obs_slot = np.array(env, np.int32), np.array(slot, np.int32)

    def _observer_index(self, like):
        """(env_of_observer [n], slot [n]) of the observers set: numpy arrays, or with torch_obs tensors beside `like`."""
        if self.torch_obs:
            import torch

            return torch.as_tensor(self._obs_env, device=like.device), torch.as_tensor(self._obs_slot, device=like.device)
        return self._obs_env, self._obs_slot

    def observe_entities(self):
        """The map observation of every observer of set_observers at the current state, with the environment's layers and
        geometry (sg_raster_map_observers): (obs [n, n_layers, n_px, n_px], env_of_observer [n], slot [n]).  torch_obs: torch
        tensors in HBM; else numpy arrays (obs bool)."""
        obs = self.engine.raster_map_observers(self._codes, self.width, self.height, self.n, self.n, torch_out=self.torch_obs)
        return (obs,) + self._observer_index(obs)

    def nearest_entities(self, k: int = 8, radius: float = float("inf")):
        """The vector observation of the ego of every environment at the current state (sg_nearest_entities): (feat [R, k, 8],
        slots [R, k] positions in scenarios[i].entities or -1, count [R]).  torch_obs: torch tensors in HBM; else numpy arrays."""
        return self._observation("nearest", False, k, radius)

    def pose_history(self, n_samples: int = 8, stride: int = 1, k: int = 0, radius: float = float("inf")):
        """The pose history of the ego of every environment at the current state (sg_pose_history): (feat [R, 1 + k, n_samples, 6],
        slots [R, k] positions in scenarios[i].entities or -1, count [R]: RolloutEngine.pose_history).  Needs the pose record
        that driver_history=... makes the engine keep.  torch_obs: torch tensors in HBM; else numpy arrays."""
        return self._observation("pose_history", False, n_samples, stride, k, radius)

    def observe_entities_nearest(self, k: int = 8, radius: float = float("inf")):
        """The vector observation of every observer of set_observers at the current state (sg_nearest_entities_observers):
        (feat [n, k, 8], slots [n, k], count [n], env_of_observer [n], slot [n]).  torch_obs: torch tensors in HBM; else numpy
        arrays."""
        return self._observation("nearest", True, k, radius)

    def range_scan(self, n_rays: int = 64, angle0: float = -np.pi, dangle: Optional[float] = None, max_range: float = 100.0):
        """The range scan of the ego of every environment at the current state (sg_range_scan): (feat [R, n_rays, 2] range and
        range rate per beam, slots [R, n_rays] positions in scenarios[i].entities or -1, hits [R]).  torch_obs: torch tensors in
        HBM; else numpy arrays."""
        return self._observation("range_scan", False, n_rays, angle0, dangle, max_range)

    def observe_entities_ranges(self, n_rays: int = 64, angle0: float = -np.pi, dangle: Optional[float] = None, max_range: float = 100.0):
        """The range scan of every observer of set_observers at the current state (sg_range_scan_observers): (feat
        [n, n_rays, 2], slots [n, n_rays], hits [n], env_of_observer [n], slot [n]).  torch_obs: torch tensors in HBM; else
        numpy arrays."""
        return self._observation("range_scan", True, n_rays, angle0, dangle, max_range)

    def surface_scan(self, layers=("driveable_surface",), n_rays: int = 64, angle0: float = -np.pi, dangle: Optional[float] = None,
                     step: float = 0.5, n_steps: int = 64, n_refine: int = 16):
        """The surface scan of the ego of every environment at the current state (sg_surface_scan): (ranges
        [R, n_layers, n_rays], flags [R, n_layers, n_rays] SURF_HIT / SURF_INSIDE, hits [R, n_layers]:
        RolloutEngine.surface_scan).  torch_obs: torch tensors in HBM; else numpy arrays."""
        return self._observation("surface_scan", False, layers, n_rays, angle0, dangle, step, n_steps, n_refine)

    def surface_scan_observers(self, layers=("driveable_surface",), n_rays: int = 64, angle0: float = -np.pi, dangle: Optional[float] = None,
                               step: float = 0.5, n_steps: int = 64, n_refine: int = 16):
        """The surface scan of every observer of set_observers at the current state (sg_surface_scan_observers): (ranges
        [n, n_layers, n_rays], flags [n, n_layers, n_rays], hits [n, n_layers], env_of_observer [n], slot [n]).  torch_obs:
        torch tensors in HBM; else numpy arrays."""
        return self._observation("surface_scan", True, layers, n_rays, angle0, dangle, step, n_steps, n_refine)

    def _set_lanes(self):
        if not self._lanes_set:
            self.engine.set_lanes(shared_lane_arrays(self.scenarios)[0])
            self._lanes_set = True

    def lane_observation(self, k: int = 3, n_ahead: int = 4, spacing: float = 2.0, radius: float = float("inf")):
        """The lane-frame vector observation of the ego of every environment at the current state (sg_lane_observation):
        (feat [R, k, 6 + 2 * n_ahead], lanes [R, k] positions in scenarios[i].road_network.lanes or -1, count [R]).  torch_obs:
        torch tensors in HBM; else numpy arrays."""
        return self._observation("lane", False, k, n_ahead, spacing, radius)

    def observe_entities_lanes(self, k: int = 3, n_ahead: int = 4, spacing: float = 2.0, radius: float = float("inf")):
        """The lane-frame vector observation of every observer of set_observers at the current state
        (sg_lane_observation_observers): (feat [n, k, 6 + 2 * n_ahead], lanes [n, k], count [n], env_of_observer [n], slot [n]).
        torch_obs: torch tensors in HBM; else numpy arrays."""
        return self._observation("lane", True, k, n_ahead, spacing, radius)

    def set_routes(self, paths=None):
        """The routes of route_observation / observe_entities_routes and of the progress reward (sg_set_routes): paths[i] =
        {entity index: polyline [n_pts, 2]} for environment i.  None: every observer and every driver (the traffic too) gets its
        own recorded trajectory.data[:, 1:3], as the traffic policy takes it.  Replaces the previous routes."""
        if paths is None:
            envs = [self._obs_env, self._trf_env] + ([self._drv_env] if self._drv_env is not None else [])
            slots = [self._obs_slot, self._trf_slot] + ([self._drv_slot] if self._drv_env is not None else [])
            pairs = sorted({(int(i), int(k)) for i, k in zip(np.concatenate(envs), np.concatenate(slots))})
            paths = [{} for _ in range(self.n_envs)]
            for i, k in pairs:
                paths[i][k] = np.asarray(self.scenarios[i].entities[k].trajectory.data, np.float64)[:, 1:3]
        elif len(paths) != self.n_envs:
            raise ValueError("set_routes: one dict of entity index -> path per environment")
        env = [i for i, d in enumerate(paths) for _ in d]
        slot = [int(k) for d in paths for k in d]
        self.engine.set_routes(env, slot, [q for d in paths for q in d.values()])
        self._routes_set = True
        if self._route_s0 is not None:  # (arclengths along other routes)
            self._route_s0[1][:] = False

    def route_observation(self, n_ahead: int = 4, spacing: float = 2.0):
        """The route and recorded-track observation of the ego of every environment at the current state
        (sg_route_observation): (feat [R, 11 + 2 * n_ahead], info [R, 2]: RolloutEngine.route_observation).  The routes are those
        of set_routes (before any: its default); an ego without one has its route part zero.  torch_obs: torch tensors in HBM;
        else numpy arrays."""
        return self._observation("route", False, n_ahead, spacing)

    def observe_entities_routes(self, n_ahead: int = 4, spacing: float = 2.0):
        """The route and recorded-track observation of every observer of set_observers at the current state
        (sg_route_observation_observers): (feat [n, 11 + 2 * n_ahead], info [n, 2], env_of_observer [n], slot [n]).  Before any
        set_routes every observer and driver gets its own recording as its route.  torch_obs: torch tensors in HBM; else numpy
        arrays."""
        return self._observation("route", True, n_ahead, spacing)

    def close(self):
        self.engine.close()
