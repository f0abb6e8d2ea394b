"""Observations of the sensors (observation.py, sensor/common.py:54-58, 109-113, sensor/map.py:21-25): dataclasses with the
reference's field names, and `combine_observations`, which CombinedSensor uses to merge the observations of several sensors
of one entity into one class."""
import dataclasses
from dataclasses import dataclass
from typing import Any, Optional, Sequence

import numpy as np


@dataclass
class Observation:
    """observation.py:10-15: base class."""


@dataclass
class SingleEntityObservation(Observation):
    """observation.py:17-28: State.get_entity_data(entity) with the entity in front."""

    entity: Any
    t: float
    next_t: float
    pose: Optional[np.ndarray]
    velocity: Optional[np.ndarray]
    distance_travelled: Optional[float]
    recorded_poses: np.ndarray
    entity_state: Any


@dataclass
class FutureCollisionObservation(SingleEntityObservation):
    """sensor/common.py:54-58."""

    future_collision: bool


@dataclass
class CollisionObservation(SingleEntityObservation):
    """sensor/common.py:109-113."""

    collisions: dict


@dataclass
class MapObservation(SingleEntityObservation):
    """sensor/map.py:21-25."""

    map: np.ndarray


@dataclass
class NearestEntitiesObservation(SingleEntityObservation):
    """The vector observation (no counterpart in the reference): `neighbours`, the nearest entities within the sensor's radius
    by ascending (squared distance, position in the scenario), at most k of them, and `features` [k, 8] -- per neighbour the
    longitudinal and lateral offset in the observer's frame, cos and sin of the relative heading, the relative velocity in
    that frame, box length and width; rows behind the last neighbour are zero."""

    neighbours: list
    features: np.ndarray


@dataclass
class PoseHistoryObservation(SingleEntityObservation):
    """The pose-history observation (no counterpart in the reference): `history` [n_samples, 6] -- where the entity itself was
    at the last n_samples rows of the pose record, `stride` rows apart, in its current frame: per sample the longitudinal and
    lateral offset, cos and sin of the heading then relative to the heading now, the age of the sample in seconds and 1.0, or
    six zeros for a sample that does not exist (before the episode began, or the entity was not in the scene then); sample 0 is
    the current state.  `history_neighbours`, the nearest entities as NearestEntitiesObservation lists them (under a name of
    its own, so that both keep their lists in a CombinedSensor), and `neighbour_histories` [k, n_samples, 6], their rows in the
    same frame; rows behind the last neighbour are zero."""

    history: np.ndarray
    history_neighbours: list
    neighbour_histories: np.ndarray


@dataclass
class LaneObservation(SingleEntityObservation):
    """The lane-frame vector observation (no counterpart in the reference): `lanes`, the lanes of the scenario's road network
    whose centre lines are nearest to the entity, within the sensor's radius, by ascending (squared distance, position in
    `RoadNetwork.lanes`), at most k of them, and `lane_features` [k, 6 + 2 * n_ahead] -- per lane the lateral offset from the
    centre line (left positive), cos and sin of the entity's heading relative to the lane direction, the arclength along the
    lane and what is left of it, the distance, then the n_ahead centre-line points ahead in the entity's frame; rows behind
    the last lane are zero."""

    lanes: list
    lane_features: np.ndarray


@dataclass
class RouteObservation:
    """The route and recorded-track observation of one entity (State.route_observation, sg_route_observation; no counterpart in
    the reference): `present` -- it is in State.poses; `features` [11 + 2 * n_ahead] -- where its own recording has it at the
    current time in its frame (2), the distance to that point, cos and sin of the recorded heading relative to its own, then
    the lateral offset from its route (left positive), cos and sin of its heading relative to the route, the arclength along
    the route, what is left of it, the distance to it, and the n_ahead route points ahead in its frame; `segment` -- the
    route segment it is nearest to (-1: no route; the route features are zero then); `recording` -- where the current time
    lies in its recording: 0 within, -1 before the first knot, 1 after the last.  `log_divergence`, `progress` and
    `remaining` name features 2, 8 and 9.  Not present: zeros, -1, -1."""

    entity: Any
    present: bool
    features: np.ndarray
    segment: int
    recording: int

    @property
    def log_divergence(self) -> float:
        return float(self.features[2])

    @property
    def progress(self) -> float:
        return float(self.features[8])

    @property
    def remaining(self) -> float:
        return float(self.features[9])


@dataclass
class RangeScanObservation(SingleEntityObservation):
    """The range scan (no counterpart in the reference): per beam of the sensor's fan `ranges`, the distance from the entity's
    pose point to the first other entity's bounding box (the sensor's max_range without a hit, 0 from inside a box),
    `range_rates`, the rate at which that distance changes (negative when the hit entity closes along the beam, 0 without a
    hit), and `hit_entities`, that entity or None."""

    ranges: np.ndarray
    range_rates: np.ndarray
    hit_entities: list


@dataclass
class SurfaceScanObservation(SingleEntityObservation):
    """The surface scan (no counterpart in the reference): per layer of the sensor's list and beam of its fan `ranges`
    [n_layers, n_rays], the distance from the entity's pose point at which the beam first changes side of the layer's surface
    -- from on it, to leaving it; from off it, to reaching it -- and the sensor's n_steps * step without a change; `hit`
    [n_layers, n_rays] bool, whether it changed side; `inside` [n_layers] bool, whether the pose point is on the layer."""

    ranges: np.ndarray
    hit: np.ndarray
    inside: np.ndarray


@dataclass
class EntityStatus:
    """The episode status of one entity (State.entity_status, sg_entity_status; the reference asks ego_collision and
    ego_off_road of entities[0] alone): `present` -- it is in State.poses; `in_collision` -- its State.collisions() row is not
    empty; `off_road` -- TERMINAL_CONDITIONS["ego_off_road"] asked of this entity (not present, or its pose point not strictly
    inside the driveable surface); `corners_on_road` -- how many of its four box corners are strictly inside it (-1 when not
    present); `layers` -- the class names of the road geometries that contain its pose point ("Road", "Intersection", "Lane",
    "Pavement", "Crossing", "Building"); `hit_entities` -- the entities of its collision row; `nearest_entity` and `clearance`
    -- the other entity whose box is nearest and the distance between the two boxes (0 when they collide; None and inf when
    it is alone); `speed`, `distance` -- |velocity[:3]| and the distance travelled.  Not present: zeros."""

    entity: Any
    present: bool
    in_collision: bool
    off_road: bool
    corners_on_road: int
    layers: list
    hit_entities: list
    nearest_entity: Any
    clearance: float
    speed: float
    distance: float


@dataclass
class TimeToCollision:
    """The time to collision of one entity (State.time_to_collision, sg_time_to_collision; no counterpart in the reference, whose
    FutureCollisionDetector replays recordings): `ttc` -- the time until its box first touches the box of another entity in
    State.poses if both keep their velocity and heading (the yaw rate is ignored), 0 for an entity it collides with already,
    inf when nothing is met within the horizon; `until` -- the time at which that overlap ends (it may be inf; 0 without a
    threat); `rel_velocity` -- the threat's velocity relative to the entity's, along and across the entity's heading (zeros
    without); `entity` -- the threat, None without; `n_contacts` -- how many entities are met within the horizon (-1 for an
    entity that is not in State.poses, whose other fields are those of "no threat" with ttc 0); `face` -- which face meets
    first: 0 the entity's front or rear, 1 its side, 2 / 3 the threat's front or rear / side, -1 for an overlap that exists
    already and without a threat."""

    ttc: float
    until: float
    rel_velocity: np.ndarray
    entity: Any
    n_contacts: int
    face: int


def combine_observations(*classes, prefixes: Optional[Sequence[Optional[str]]] = None):
    """observation.py:31-84: a dataclass holding the fields of all `classes` in order.  A field name that an earlier class
    already contributed is skipped -- or, with `prefixes` (one per class), taken as "<prefix>_<name>"; a name that is still
    taken then is an error.  The class has `from_obs(*observations)`, which builds it from one instance per input class."""
    if prefixes is not None and len(prefixes) != len(classes):
        raise ValueError("one prefix per observation class")
    fields, sources = [], []  # (name, type), (index of the class, its own field name)
    taken = set()
    for k, c in enumerate(classes):
        if not dataclasses.is_dataclass(c):
            raise TypeError(f"Observation {c} is not a dataclass.")
        for f in dataclasses.fields(c):
            name = f.name
            if name in taken:
                if prefixes is None:
                    continue
                name = f"{prefixes[k]}_{f.name}"
                if name in taken:
                    raise ValueError(f"Prefix {prefixes[k]} still leads to a duplicate name for {name}.")
            taken.add(name)
            fields.append((name, f.type))
            sources.append((k, f.name))

    def from_obs(cls, *obs):
        return cls(*(getattr(obs[k], name) for k, name in sources))

    return dataclasses.make_dataclass("CombinedObservation", fields, bases=(Observation,),
                                      namespace={"from_obs": classmethod(from_obs)})
