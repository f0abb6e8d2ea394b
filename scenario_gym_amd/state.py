"""State: read-only view of one scenario of a device batch with the reference's State read API
(scenario_gym/state/state.py:20-395).  Values are fetched from HBM on demand and cached per step."""
from typing import Dict, List, Optional

import numpy as np

from . import _lib as L
from .entity import Entity
from .observation import EntityStatus, RouteObservation, TimeToCollision
from .road_network import LAYER_CROSSING, LAYER_IMPENETRABLE, LAYER_INTERSECTION, LAYER_LANE, LAYER_PAVEMENT, LAYER_ROAD
from .scenario import Scenario

# the class names State.get_road_info_at_entity gives the geometries of each layer (EntityStatus.layers)
LAYER_CLASS_NAMES = ((LAYER_ROAD, "Road"), (LAYER_INTERSECTION, "Intersection"), (LAYER_LANE, "Lane"), (LAYER_PAVEMENT, "Pavement"),
                     (LAYER_CROSSING, "Crossing"), (LAYER_IMPENETRABLE, "Building"))


class State:
    def __init__(self, gym, index: int, scenario: Scenario, agents: dict, persist: bool):
        self._gym, self._i = gym, index
        self._scenario = scenario
        self.agents = agents
        self.persist = persist
        self.scenario_path: Optional[str] = None
        self.last_keystroke = None
        self.state_callbacks = []
        self._prev_poses_arr = None
        self._t_replay = None  # the clock value update_actions sees while a device rollout's actions are replayed
        self._reset_actions()

    # ------------------------------------------------------------------ scenario actions (state/state.py:150-160, 241-266)
    def _reset_actions(self) -> None:
        """State._reset_data: every action of the scenario is unapplied again, no entity has a state."""
        self.unapplied_actions = list(self._scenario.actions)
        self.action_apply_times = {a: float("nan") for a in self._scenario.actions}
        self.entity_state = dict.fromkeys(self._scenario.entities)

    def update_actions(self) -> None:
        """state.py:241-251: apply the actions whose trigger holds now, in the scenario's order; keep the others."""
        unapplied = []
        for act in self.unapplied_actions:
            if act.trigger_condition(self):
                self.apply_action(act)
                self.action_apply_times[act] = self.t
            else:
                unapplied.append(act)
        self.unapplied_actions = unapplied

    def apply_action(self, action) -> None:
        """state.py:253-262."""
        import warnings

        entity = self._scenario.entity_by_name(action.entity_ref)
        if entity is None:
            warnings.warn(f"No entity with name {action.entity_ref} was found for action {action.__class__.__name__}.")
        else:
            action.apply(self, entity)

    def _replay_actions(self, clock) -> None:
        """update_actions() once per value of `clock` (State.t after each step of a device call that ran several steps at
        once): what stepping one by one would have done, for actions whose trigger reads nothing but State.t."""
        if not self.unapplied_actions:
            return
        try:
            for t in clock:
                self._t_replay = float(t)
                self.update_actions()
                if not self.unapplied_actions:
                    break
        finally:
            self._t_replay = None

    # ------------------------------------------------------------------ plumbing
    def _s(self):
        return self._gym._fetch_state()

    def get_callback(self, cls):
        """state/state.py:272-282: the state callback of class `cls`, or None."""
        for cb in self._gym.state_callbacks:
            if isinstance(cb, cls):
                return cb
        return None

    @property
    def scenario(self) -> Scenario:
        return self._scenario

    @property
    def all_entities(self) -> List[Entity]:
        return list(self._scenario.entities)

    def _dict(self, arr) -> Dict[Entity, np.ndarray]:
        s = self._s()
        pres = s["present"][self._i]
        return {e: arr[self._i, k].copy() for k, e in enumerate(self._scenario.entities) if pres[k]}

    # ------------------------------------------------------------------ reference read API
    @property
    def t(self) -> float:
        if self._t_replay is not None:
            return self._t_replay
        return float(self._s()["t"][self._i])

    @property
    def prev_t(self) -> float:
        return float(self._s()["prev_t"][self._i])

    @property
    def dt(self) -> float:
        return self.t - self.prev_t

    @property
    def next_t(self) -> float:
        return self.t + self._gym.timestep

    @property
    def is_done(self) -> bool:
        return bool(self._s()["done"][self._i])

    def terminal_condition(self, name: str) -> bool:
        """TERMINAL_CONDITIONS[name](state) of the reference (state.py:397-408) on the current state, whatever the gym's own
        terminal_conditions are: all four are evaluated on the device for every scenario (sg_terminal_flags; ego_off_road
        against the scenario's road network -- none: off the road)."""
        from .engine import TERMINAL_BITS

        if name == "ego_off_road":
            self._gym._set_road_networks()
        return bool(self._gym._terminal_flags()[self._i] & TERMINAL_BITS[name])

    @property
    def poses(self) -> Dict[Entity, np.ndarray]:
        return self._dict(self._s()["poses"])

    @property
    def velocities(self) -> Dict[Entity, np.ndarray]:
        return self._dict(self._s()["vels"])

    @property
    def prev_poses(self) -> Dict[Entity, np.ndarray]:
        """poses - velocities * dt is NOT used: the previous step's poses are kept by the gym."""
        prev = self._gym._prev_state
        if prev is None:
            return {}
        now = self._s()["present"][self._i]
        return {e: prev["poses"][self._i, k].copy() for k, e in enumerate(self._scenario.entities)
                if now[k] and prev["present"][self._i, k]}

    @property
    def distances(self) -> Dict[Entity, float]:
        d = self._s()["dists"][self._i]
        return {e: float(d[k]) for k, e in enumerate(self._scenario.entities)}

    def collisions(self) -> Dict[Entity, List[Entity]]:
        """State.collisions() (state.py:306-310): adjacency rows computed on the device."""
        s = self._s()
        ents = self._scenario.entities
        rows, pres = s["coll"][self._i], s["present"][self._i]
        rows = rows.reshape(len(rows), -1)  # [E, words]: one 64-bit word per 64 entity slots (scenarios of any width)

        def listed(k):
            return [ents[j] for j in range(len(ents)) if (int(rows[k, j >> 6]) >> (j & 63)) & 1]

        return {e: listed(k) for k, e in enumerate(ents) if pres[k]}

    def recorded_poses(self, entity: Optional[Entity] = None):
        """state.py:272-290: (n, 7) rows [t, x, y, z, h, p, r] of the steps the entity was present."""
        t, poses = self._gym._fetch_record()
        ents = self._scenario.entities
        rows = int(self._s()["n_steps"][self._i]) + 1  # a scenario that ended before the batch did has no later rows

        def one(k):
            p = poses[:rows, self._i, k]
            ok = ~np.isnan(p[:, 0])
            return np.concatenate([t[:rows][ok, self._i, None], p[ok]], axis=1) if ok.any() else np.empty((0, 7))

        if entity is not None:
            return one(ents.index(entity))
        return {e: one(k) for k, e in enumerate(ents)}

    def get_entity_data(self, entity: Entity):
        """state.py:292-304."""
        return (self.t, self.next_t, self.poses.get(entity), self.velocities.get(entity),
                self.distances.get(entity), self.recorded_poses(entity=entity), self.entity_state.get(entity, None))

    def get_entity_box_points(self, e: Entity) -> np.ndarray:
        return e.get_bounding_box_points(self.poses[e])

    def _sensor_row(self, entity: Optional[Entity]):
        """(observers, row) of the gym's sensor results for `entity`: the per-scenario calls and this scenario's row for the
        ego, else the observer-list calls and the entity's place in the gym's observer list."""
        if entity is None or entity is self._scenario.ego:
            return False, self._i
        return True, self._gym._observer(self._i, self._scenario.entities.index(entity))

    def future_collision(self, horizon: float = 5.0, n_samples: int = 10, entity: Optional[Entity] = None) -> bool:
        """FutureCollisionDetector(entity, horizon) at the current time (sensor/common.py:87-106), computed on the device;
        entity: any entity of the scenario (default: the ego)."""
        observers, row = self._sensor_row(entity)
        return bool(self._gym._observation("future", observers, float(horizon), int(n_samples))[row])

    def entity_raster(self, width: float = 20.0, height: float = 20.0, nw: int = 20, nh: int = 20) -> np.ndarray:
        """RasterizedMapSensor "entity" layer around the ego (sensor/map.py:120-192), computed on the device: bool [nh, nw]."""
        return self._gym._raster(float(width), float(height), int(nw), int(nh))[self._i]

    def raster_map(self, layers, width: float = 20.0, height: float = 20.0, nw: int = 20, nh: int = 20,
                   entity: Optional[Entity] = None) -> np.ndarray:
        """RasterizedMapSensor layers around `entity` -- any entity of the scenario, default the ego (sensor/map.py:136-271;
        names of its `_all_layers`) -- computed on the device from the scenario's road network: bool [n_layers, nh, nw]; all
        False for an entity that is not in `poses`."""
        observers, row = self._sensor_row(entity)
        return self._gym._raster_map(observers, tuple(layers), float(width), float(height), int(nw), int(nh))[row]

    def nearest_entities(self, k: int = 8, radius: float = float("inf"), entity: Optional[Entity] = None):
        """NearestEntitiesSensor(entity, k, radius) at the current state, computed on the device: (neighbours, features) -- the
        at most k nearest other entities in `poses` within `radius` of `entity` (any entity of the scenario, default the ego)
        by ascending (squared distance, position in the scenario), and their [k, 8] feature rows in the entity's frame (zeros
        behind the last).  ([], zeros) for an entity that is not in `poses`."""
        observers, row = self._sensor_row(entity)
        feat, slots, _ = self._gym._observation("nearest", observers, int(k), float(radius))
        ents = self._scenario.entities
        return [ents[j] for j in slots[row] if j >= 0], feat[row].copy()

    def pose_history(self, n_samples: int = 8, stride: int = 1, k: int = 0, radius: float = float("inf"),
                     entity: Optional[Entity] = None):
        """PoseHistorySensor(entity, n_samples, stride, k, radius) at the current state, computed on the device from the pose
        record (sg_pose_history; needs the gym's record=True): (history [n_samples, 6], neighbours, neighbour_histories
        [k, n_samples, 6]) -- where `entity` (any entity of the scenario, default the ego) and the at most k entities
        nearest_entities(k, radius) lists were at the last n_samples record rows, `stride` rows apart, in the entity's current
        frame: per sample the longitudinal and lateral offset, cos and sin of the relative heading, the age in seconds and 1.0;
        six zeros for a sample from before the episode began, for an entity that was not in `poses` then, and behind the last
        neighbour.  (zeros, [], zeros) for an entity that is not in `poses`."""
        observers, row = self._sensor_row(entity)
        feat, slots, _ = self._gym._observation("pose_history", observers, int(n_samples), int(stride), int(k), float(radius))
        ents = self._scenario.entities
        return feat[row, 0].copy(), [ents[j] for j in slots[row] if j >= 0], feat[row, 1:].copy()

    def range_scan(self, n_rays: int = 64, angle0: float = -np.pi, dangle: Optional[float] = None, max_range: float = 100.0,
                   entity: Optional[Entity] = None):
        """RangeScanSensor(entity, n_rays, angle0, dangle, max_range) at the current state, computed on the device: (ranges
        [n_rays], range_rates [n_rays], hit_entities) -- per beam from the pose point of `entity` (any entity of the scenario,
        default the ego), at the angle angle0 + b * dangle from its heading (dangle None: 2 pi / n_rays), the distance to the
        first other entity's bounding box within max_range (max_range without a hit), the rate at which it changes, and that
        entity (None without a hit).  (zeros, zeros, Nones) for an entity that is not in `poses`."""
        observers, row = self._sensor_row(entity)
        feat, slots, _ = self._gym._observation("range_scan", observers, int(n_rays), float(angle0), None if dangle is None else float(dangle),
                                                float(max_range))
        ents = self._scenario.entities
        return feat[row, :, 0].copy(), feat[row, :, 1].copy(), [ents[j] if j >= 0 else None for j in slots[row]]

    def surface_scan(self, layers=("driveable_surface",), n_rays: int = 64, angle0: float = -np.pi, dangle: Optional[float] = None,
                     step: float = 0.5, n_steps: int = 64, n_refine: int = 16, entity: Optional[Entity] = None):
        """SurfaceScanSensor(entity, layers, n_rays, angle0, dangle, step, n_steps, n_refine) at the current state, computed on the
        device against the scenario's road network: (ranges [n_layers, n_rays], hit [n_layers, n_rays] bool, inside [n_layers]
        bool) -- per layer (names of RasterizedMapSensor's surface layers, "impenetrable", or LAYER_* bits) and beam from the pose
        point of `entity` (any entity of the scenario, default the ego), the beams of range_scan, the range at which the beam
        first changes side of the layer's surface (n_steps * step without a change), whether it did, and whether the pose point
        is on the layer.  (zeros, False, False) for an entity that is not in `poses`."""
        from .road_network import surface_layer_bits

        observers, row = self._sensor_row(entity)
        feat, flags, _ = self._gym._surface_scan(observers, tuple(surface_layer_bits(layers)), int(n_rays), float(angle0),
                                                 None if dangle is None else float(dangle), float(step), int(n_steps), int(n_refine))
        return feat[row].copy(), (flags[row] & L.SURF_HIT) != 0, (flags[row, :, 0] & L.SURF_INSIDE) != 0

    def entity_status(self, entity: Optional[Entity] = None):
        """The episode status of `entity` (any entity of the scenario, default the ego) at the current state, computed on the
        device (sg_entity_status / sg_entity_status_observers): an EntityStatus -- in the scene, in a collision and with whom,
        off the road, box corners on the road, the road geometry classes under it, the nearest other box and the clearance
        to it, speed and distance travelled."""
        observers, row = self._sensor_row(entity)
        flags, info, feat = self._gym._observation("entity_status", observers)
        ents = self._scenario.entities
        entity = self._scenario.ego if entity is None else entity
        f, near = int(flags[row]), int(info[row, 3])
        present = bool(f & L.ST_PRESENT)
        return EntityStatus(entity, present, bool(f & L.ST_COLLISION), bool(f & L.ST_OFF_ROAD), int(info[row, 2]),
                            [name for bit, name in LAYER_CLASS_NAMES if (f >> L.ST_LAYER_SHIFT) & bit],
                            list(self.collisions().get(entity, [])) if present else [], ents[near] if near >= 0 else None,
                            float(feat[row, 2]), float(feat[row, 0]), float(feat[row, 1]))

    def lane_observation(self, k: int = 3, n_ahead: int = 4, spacing: float = 2.0, radius: float = float("inf"),
                         entity: Optional[Entity] = None):
        """LaneSensor(entity, k, n_ahead, spacing, radius) at the current state, computed on the device: (lanes, features) -- the
        at most k lanes of the scenario's road network (objects of `RoadNetwork.lanes`) whose centre lines are nearest to
        `entity` (any entity of the scenario, default the ego) and within `radius`, by ascending (squared distance, position in
        `RoadNetwork.lanes`), and their [k, 6 + 2 * n_ahead] feature rows (zeros behind the last).  ([], zeros) for an entity
        that is not in `poses` and for a scenario without a road network."""
        observers, row = self._sensor_row(entity)
        feat, idx, _ = self._gym._observation("lane", observers, int(k), int(n_ahead), float(spacing), float(radius))
        rn = self._scenario.road_network
        lanes = rn.lanes if rn is not None else []
        return [lanes[j] for j in idx[row] if j >= 0], feat[row].copy()

    def route_observation(self, n_ahead: int = 4, spacing: float = 2.0, entity: Optional[Entity] = None):
        """The route and recorded-track observation of `entity` (any entity of the scenario, default the ego) at the current
        state, computed on the device (sg_route_observation / sg_route_observation_observers): a RouteObservation -- how far
        the entity is from where its own recording has it, and where it is along its route with n_ahead points of the route
        ahead.  The routes are those of ScenarioGym.set_routes; by default every entity's own recorded trajectory."""
        observers, row = self._sensor_row(entity)
        feat, info = self._gym._observation("route", observers, int(n_ahead), float(spacing))
        entity = self._scenario.ego if entity is None else entity
        present = bool(self._s()["present"][self._i, self._scenario.entities.index(entity)])
        return RouteObservation(entity, present, feat[row].copy(), int(info[row, 0]), int(info[row, 1]))

    def time_to_collision(self, entity: Optional[Entity] = None, horizon: float = float("inf")):
        """The time to collision of `entity` (any entity of the scenario, default the ego) at the current state, computed on the
        device (sg_time_to_collision / sg_time_to_collision_observers): a TimeToCollision -- when its box first touches the box
        of another entity within `horizon` seconds if both keep their velocity and heading, until when, that entity, its
        relative velocity in the entity's frame, how many entities are met, and the face that meets first."""
        observers, row = self._sensor_row(entity)
        feat, info = self._gym._observation("ttc", observers, float(horizon))
        ents = self._scenario.entities
        threat = int(info[row, 0])
        return TimeToCollision(float(feat[row, 0]), float(feat[row, 1]), feat[row, 2:4].copy(), ents[threat] if threat >= 0 else None,
                               int(info[row, 1]), int(info[row, 2]))

    def get_road_info_at_entity(self, e: Entity):
        """state.py:330-338: (class names, objects) of the road geometries whose boundary strictly contains the entity's
        position -- "Road", "Intersection", "Lane", "Pavement", "Crossing", "Building", the objects the scenario's RoadNetwork
        holds, in `road_network_geometries` order.  ([], []) without a road network; KeyError for an entity that is not in
        `poses`.  Computed on the device for every entity of the batch at once (sg_road_info), cached per state."""
        k = self._scenario.entities.index(e) if e in self._scenario.entities else -1
        if k < 0 or not self._s()["present"][self._i, k]:
            raise KeyError(e)
        rn = self._scenario.road_network
        if not rn:
            return [], []
        count, geoms, _ = self._gym._road_info()
        objs = [rn.geometry_index()[j] for j in geoms[self._i, k, :count[self._i, k]]]
        return [o.__class__.__name__ for o in objs], objs

    def get_entities_in_area(self, area) -> List[Entity]:
        """state.py:340-354: entities whose centre point lies strictly inside `area`.  The reference takes a shapely
        (Multi)Polygon; here `area` is anything with `.exterior.coords`, or an (n, 2) array of ring vertices (simple
        polygon, either orientation; holes are not supported)."""
        ring = np.asarray(area.exterior.coords if hasattr(area, "exterior") else area, np.float64)[:, :2]
        if len(ring) > 1 and np.array_equal(ring[0], ring[-1]):
            ring = ring[:-1]
        ax, ay = ring[:, 0], ring[:, 1]
        bx, by = np.roll(ax, -1), np.roll(ay, -1)
        out = []
        for e, pose in self.poses.items():
            px, py = pose[0], pose[1]
            cr = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
            on_edge = (cr == 0) & (np.minimum(ax, bx) <= px) & (px <= np.maximum(ax, bx)) & \
                      (np.minimum(ay, by) <= py) & (py <= np.maximum(ay, by))
            if on_edge.any():
                continue  # shapely `contains`: boundary points are outside
            cross = ((ay > py) != (by > py)) & (px < (bx - ax) * (py - ay) / np.where(by == ay, 1.0, by - ay) + ax)
            if cross.sum() % 2 == 1:
                out.append(e)
        return out

    def to_scenario(self, name: Optional[str] = None) -> Scenario:
        """state.py:374-394: a scenario whose trajectories are the recorded poses (stationary entities keep one
        knot).  Needs the gym's pose record (`record=True`, the default of ScenarioGym)."""
        from copy import deepcopy

        from .trajectory import Trajectory, is_stationary

        if name is None:
            name = f"Simulation of {self.scenario.name}" if self.scenario.name is None else None
        entities = []
        for entity, poses in self.recorded_poses().items():
            new_entity = deepcopy(entity)
            if is_stationary(poses):
                poses = poses[None, 0]
            new_entity.trajectory = Trajectory(poses)
            entities.append(new_entity)
        return Scenario(entities, name=name, road_network=self.scenario.road_network, actions=self.scenario.actions)

    def get_entities_in_radius(self, x: float, y: float, r: float) -> List[Entity]:
        """state.py:356-372.  The reference tests the centre against the 64-gon Point(x, y).buffer(r)."""
        ang = 2.0 * np.pi * np.arange(64) / 64
        vx, vy = x + r * np.cos(ang), y - r * np.sin(ang)
        out = []
        for e, pose in self.poses.items():
            ex, ey = np.roll(vx, -1) - vx, np.roll(vy, -1) - vy
            cr = ex * (pose[1] - vy) - ey * (pose[0] - vx)
            if (cr < 0).all():  # clockwise ring: strictly inside
                out.append(e)
        return out


# state.py:397-408: name -> predicate over a State, as the reference's callers index it (TERMINAL_CONDITIONS["collision"](state));
# ScenarioGym(terminal_conditions=[...]) takes the names (evaluated inside the rollout kernels) or any callable (host, per step).
TERMINAL_CONDITIONS = {name: (lambda s, _n=name: s.terminal_condition(_n))
                       for name in ("max_length", "collision", "ego_collision", "ego_off_road")}
