/*
 * sgym.h -- C ABI of libsgym_hip.so: the MI355X (gfx950) batched scenario-rollout engine.
 *
 * The reference (driskai/scenario_gym v0.3.1) is pure Python and has no FFI; its extension surface
 * for the per-step hot path is Python subclassing.  This header is the device boundary the build
 * introduces at the ScenarioGym <-> (agents + State + metrics) seam; every entry point names the
 * reference interface it stands in for (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 (SG_OK) or a negative sg_status.
 *   - the caller owns every host buffer it passes; the library owns all device memory and one HIP
 *     stream per handle.  Device pointers returned by sg_state_view stay valid until sg_upload /
 *     sg_destroy on that handle.
 *   - a handle is bound to one device and is not thread-safe; different handles may be driven
 *     from different host threads.  Calls are synchronous on return unless documented otherwise.
 *   - R = scenarios (replicas) on this handle, E = entity slots per scenario (ragged scenarios
 *     pad with SG_KIND_NONE), poses are fp64 [x, y, z, h, p, r] exactly as in the reference.
 */
#ifndef SGYM_H
#define SGYM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_ABI_VERSION 7 /* 2: sg_scenario_state.last_row_hi (scenarios of up to 512 entities); 3: sg_schedule_info replaces sg_pipeline_info; 4: sg_crowd_walk_stats removed; 5: sg_last_kernel; 6: sg_road_info, sg_road_info_points; 7: sg_set_observers, sg_raster_map_observers, sg_future_collision_observers (added within 7, purely additive: sg_nearest_entities, sg_nearest_entities_observers; sg_set_lanes, sg_lane_observation, sg_lane_observation_observers; sg_range_scan, sg_range_scan_observers; sg_set_drivers, sg_step_drivers; sg_entity_status, sg_entity_status_observers; sg_set_driver_policy, sg_driver_policy_actions, sg_step_drivers_policy; sg_snapshot_create, sg_snapshot_save, sg_snapshot_restore, sg_snapshot_bytes, sg_snapshot_destroy) */

typedef enum {
    SG_OK = 0,
    SG_ERR_INVALID = -1,   /* bad argument */
    SG_ERR_HIP = -2,       /* HIP runtime error, see sg_last_error */
    SG_ERR_STATE = -3,     /* call order (e.g. step before upload) */
    SG_ERR_NO_DEVICE = -4, /* no gfx950 device visible */
    SG_ERR_CAPACITY = -5,  /* record / event capacity exceeded */
} sg_status;

/* how an entity slot gets its next pose (ScenarioGym.create_agents, scenario_gym/scenario_gym.py:188-211) */
typedef enum {
    SG_KIND_NONE = 0,          /* padding, never present */
    SG_KIND_REPLAY = 1,        /* non-agent: BatchReplayEntity, scenario_gym/entity/batch.py:34-128 */
    SG_KIND_AGENT_REPLAY = 2,  /* ReplayTrajectoryAgent + ReplayTrajectoryController, agent.py:118-128, controller.py:45-54 */
    SG_KIND_AGENT_PID = 3,     /* PIDAgent + PIDController, agent.py:131-148, controller.py:143-258 */
    SG_KIND_AGENT_VEHICLE = 4, /* external (accel, steer) -> VehicleController, controller.py:57-140; integrations/openaigym.py:197-204 */
    SG_KIND_AGENT_PEDESTRIAN = 5, /* PedestrianAgent + SocialForce + PedestrianController, pedestrian/{agent,social_force,controller}.py */
    SG_KIND_AGENT_EXTERNAL = 6,   /* any other Agent subclass (agent.py:18-116): agent.step(state) runs in the caller, one
                                     sg_step per tick, and its pose enters through sg_set_external_poses */
} sg_kind;

/* TERMINAL_CONDITIONS, scenario_gym/state/state.py:397-408 */
#define SG_TERM_MAX_LENGTH 1u
#define SG_TERM_COLLISION 2u
#define SG_TERM_EGO_COLLISION 4u
#define SG_TERM_EGO_OFF_ROAD 8u /* entities[0] absent or not strictly inside RoadNetwork.driveable_surface (sg_set_road_networks);
                                   with pedestrian agents in the batch: a launch of its own behind every step */

/* The unions of RoadGeometry boundaries the reference takes: RoadNetwork.driveable_surface / walkable_surface /
 * impenetrable_surface (road_network/road_network.py:306-328, flags in road_network/objects.py) and the per-layer
 * unions of RasterizedMapSensor (sensor/map.py:194-271).  A polygon carries the bits of every union it is part of. */
#define SG_LAYER_DRIVEABLE 1u    /* roads, intersections and all lanes */
#define SG_LAYER_ROAD 2u
#define SG_LAYER_INTERSECTION 4u
#define SG_LAYER_LANE 8u         /* the lanes of the roads */
#define SG_LAYER_WALKABLE 16u    /* pavements, crossings, buildings */
#define SG_LAYER_PAVEMENT 32u
#define SG_LAYER_CROSSING 64u
#define SG_LAYER_IMPENETRABLE 128u

/* The boundary polygons of the scenarios' road networks (Scenario.road_network; JSON format of
 * road_network/utils.py:6-41).  Networks are shared: scenario r uses network net_of_scenario[r] (-1: none, every
 * surface empty).  Polygon q of network n = polygons [poly_off[n], poly_off[n+1]); its rings (exterior first, then
 * holes) = rings [ring_off[q], ring_off[q+1]); ring vertices = verts[vert_off[ring] .. vert_off[ring+1]), rings OPEN
 * (last vertex != first).  HOST arrays, copied by the call. */
typedef struct sg_road_networks {
    int32_t n_networks;
    const int32_t *net_of_scenario; /* [n_scenarios] */
    const int64_t *poly_off;        /* [n_networks + 1] */
    const int64_t *ring_off;        /* [n_polygons + 1] */
    const int64_t *vert_off;        /* [n_rings + 1] */
    const double *verts;            /* [n_verts][2] x, y */
    const uint32_t *layers;         /* [n_polygons] SG_LAYER_* */
} sg_road_networks;

/* The lane centre lines of the same networks (Lane.center and Lane.successors, road_network/objects.py), for
 * sg_lane_observation.  Lane q of network n = lanes [lane_off[n], lane_off[n+1]); its centre points =
 * pts[pt_off[q] .. pt_off[q+1]) in driving order (fewer than two points: the lane has no segments and is never chosen);
 * its successors = succ[succ_off[q] .. succ_off[q+1]), lane indices WITHIN the network (the library sorts them and drops
 * duplicates).  HOST arrays, copied by the call. */
typedef struct sg_lanes {
    int32_t n_networks;
    const int64_t *lane_off; /* [n_networks + 1] */
    const int64_t *pt_off;   /* [n_lanes + 1] */
    const double *pts;       /* [n_pts][2] x, y */
    const int64_t *succ_off; /* [n_lanes + 1] */
    const int32_t *succ;     /* [n_succ] */
} sg_lanes;

/* controller parameter slots (VehicleController.__init__ controller.py:64-98, PIDController.__init__ :154-196) */
enum {
    SG_C_MAX_STEER = 0,
    SG_C_MAX_ACCEL = 1,
    SG_C_MAX_SPEED = 2, /* NaN = None */
    SG_C_ALLOW_REVERSE = 3,
    SG_C_STEER_KP = 4,
    SG_C_STEER_KD = 5,
    SG_C_ACCEL_KP = 6,
    SG_C_ACCEL_KD = 7,
    SG_C_ACCEL_KI = 8,
    /* PedestrianAgent / PedestrianSensor / PedestrianController (pedestrian/agent.py:18-37, controller.py:12-19) */
    SG_C_PED_SPEED_DESIRED = 9,
    SG_C_PED_MAX_SPEED = 10,
    SG_C_PED_HEAD_ROT = 11,
    SG_C_PED_RADIUS = 12, /* PedestrianSensor.distance_threshold */
    SG_NCTRL = 16
};

/* ScenarioGym.__init__(timestep, persist, terminal_conditions), scenario_gym/scenario_gym.py:29-95 */
typedef struct {
    int32_t device;          /* HIP device ordinal */
    int32_t n_scenarios;     /* R */
    int32_t n_entities;      /* E, entity slots per scenario (the reference has no ceiling, state/utils.py:10-49; here <= 16384).
                                Up to 512: one workgroup per scenario, every kind, callback and observation call.  Beyond: the
                                step runs as four kernels over as many workgroups as the scenario needs -- every entity kind
                                (caller-run agents; pedestrian agents with the counter-based noise), the RSS callback (a launch
                                of its own per step), road networks with ego_off_road, the pedestrians' boundary forces and the
                                map's surface layers, both noise modes, several pedestrian models, the observation calls and
                                sg_tick: nothing is refused at that width */
    int32_t persist;         /* ScenarioGym(persist=...) */
    uint32_t terminal_mask;  /* SG_TERM_* */
    int32_t record_capacity; /* rows of State._recorded_poses kept on device (0 = off), state.py:227-228 */
    int32_t event_capacity;  /* CollisionMetric events kept per scenario (metrics/collision.py:70-75); later events are
                                counted in sg_metrics.n_collisions but not stored */
    int32_t reserved;
    double timestep;         /* ScenarioGym(timestep=...) */
} sg_config;

/* Numeric content of R scenarios: what State/Entity/Trajectory objects hold after load.
 * All pointers are HOST pointers, entity index i = scenario*E + slot. */
typedef struct {
    const int32_t *kind;     /* [R*E] sg_kind */
    const int32_t *etype;    /* [R*E] catalog type: 0 Vehicle, 1 Pedestrian, 2 other (metrics/collision.py:85) */
    const double *bbox;      /* [R*E][4] BoundingBox width, length, center_x, center_y (catalog_entry.py:83-91) */
    const int64_t *knot_off; /* [R*E+1] row offsets into knots (empty range for SG_KIND_NONE) */
    const double *knots;     /* [rows][7] Trajectory.data rows t,x,y,z,h,p,r (trajectory.py:91) */
    const double *ctrl;      /* [R*E][SG_NCTRL] or NULL for the reference defaults */
    const int32_t *ego;      /* [R] slot of Scenario.ego (scenario/scenario.py:53-65) */
    const double *t0;        /* [R] ScenarioGym.get_start_time (scenario_gym.py:213-215) */
    const double *length;    /* [R] Scenario.length (scenario/scenario.py:88-91) */
    const int64_t *route_off; /* [R*E+1] row offsets into routes, or NULL when there are no pedestrian agents */
    const double *routes;     /* [rows][2] PedestrianAgent.route waypoints (pedestrian/agent.py:43) */
} sg_scenarios;

/* SocialForceParameters (pedestrian/social_force.py:16-30; behaviour.py max_speed_factor; random_walk.py bias):
 * one set per handle.  The Gaussian noise terms (std_lon, std_lat; social_force.py:106-108) are set with
 * sg_set_ped_noise; without that call they are off (std 0: np.random.normal(b, 0) == b). */
typedef struct {
    double relaxation_time, ped_repulse_V, ped_repulse_sigma, ped_attract_C;
    double sight_weight, sight_weight_use;
    double cos_sight;        /* cos(sight_angle / 2 * pi / 180), computed by the caller */
    double max_speed_factor, bias_lon, bias_lat;
    /* repulsion from the impenetrable surface (buildings) of the scenario's road network, social_force.py:97-104; acts
     * when sg_set_road_networks has been called.  (The "walkable boundary" term :86-95 is evaluated only for a pedestrian
     * inside the walkable surface, where shapely's nearest point is the pedestrian itself: it is the zero vector whatever
     * boundary_repulse_U / R are, so they are not parameters here.) */
    double imp_boundary_repulse_U, imp_boundary_repulse_R;
} sg_social_force;

/* Device-resident state after the latest step: the arrays behind State.poses / velocities /
 * distances / collisions() (state.py:90-96, 306-310).
 *
 * Layout: entity slot i = scenario * entity_stride + slot.  Entities are grouped in blocks of 64
 * consecutive slots (the 64 lanes of one gfx950 wavefront); inside a block every field is one row of
 * 64 eight-byte values, so a wavefront loads/stores whole 512-byte rows:
 *     value(field f, entity i) = blocks[(i / 64) * block_rows * 64 + f * 64 + (i % 64)]
 * block_rows = SG_F_COLL + row_words, row_words = ceil(entity_stride / 64) (1 for up to 64 entities).
 * Raw device pointers (wrap with torch/dlpack for zero-copy strided views). */
enum {
    SG_F_POSE = 0,      /* 6 rows: x, y, z, h, p, r  (State.poses) */
    SG_F_VEL = 6,       /* 6 rows (State.velocities) */
    SG_F_DIST = 12,     /* State.distances */
    SG_F_PRESENT = 13,  /* uint64 0/1: entity in State.poses */
    SG_F_CTRL = 14,     /* 4 rows: controller speed, e_lon_prev, e_lat_prev, e_lon_int (controller.py:100-103,198-203);
                           pedestrians: controller speed, goal_idx (pedestrian/controller.py:21-23, agent.py:38) */
    SG_F_FORCE = 18,    /* 2 rows: PedestrianAgent.force (pedestrian/agent.py:41, social_force.py:114) */
    SG_F_COLL = 20      /* row_words rows of uint64: adjacency row of State.collisions(), bit j = slot j of the scenario */
};

/* per-scenario clock, terminal flag and metric accumulators */
typedef struct {
    double t, prev_t;              /* State.t, State.prev_t */
    double ego_avg_speed;          /* EgoAvgSpeed (metrics/trajectory.py:8-28) */
    double ego_max_speed;          /* EgoMaxSpeed (:31-48) */
    double avg_t;                  /* EgoAvgSpeed.t */
    double ego_distance_travelled; /* EgoDistanceTravelled (:51-66) */
    uint64_t last_row[4];          /* CollisionMetric.last_timestep (metrics/collision.py:75) */
    int32_t done;                  /* State.is_done */
    int32_t n_steps;               /* steps since reset */
    int32_t n_events;              /* len(CollisionMetric.collisions) */
    int32_t rec_rows;              /* rows written to the pose record */
    int64_t noise_pos;             /* variates of the scenario's noise stream consumed so far (sg_set_ped_noise, SG_NOISE_STREAM) */
    uint64_t last_row_hi[4];       /* words 4..7 of last_row (scenarios of 257..512 entities; beyond 512 the rows live in
                                      sg_handle scratch, sgym_wide.hpp) */
} sg_scenario_state;               /* 136 bytes */

typedef struct {
    int32_t n_scenarios, n_entities, entity_stride, n_blocks;
    int32_t row_words, block_rows;
    double *blocks;          /* [n_blocks][block_rows][64] */
    sg_scenario_state *scen; /* [n_scenarios] */
} sg_state_view;

/* per-scenario metric row: EgoAvgSpeed/EgoMaxSpeed/EgoDistanceTravelled (metrics/trajectory.py:8-66),
 * CollisionMetric count (metrics/collision.py:46-79), plus bookkeeping */
typedef struct {
    double ego_avg_speed, ego_max_speed, ego_distance_travelled;
    double final_t;
    int32_t n_steps, done, n_collisions, reserved;
} sg_metrics;

/* one CollisionMetric entry (t, other entity, type): metrics/collision.py:81-203.  type = CollisionTypes: 0 other,
 * 1 t_bone, 2 head_on, 3 rear_end, 4 side_swipe, 5 non_vehicle (hazard's catalog type is not "Vehicle").  Vehicle hazards
 * are classified by record_collision's tree with state.poses[...] where the reference writes the (missing) `.pose`
 * attribute; the classification runs when the events are read (sg_read_metrics) from the ego pose the library keeps with
 * every event (device side) and the hazard's pose at time t re-evaluated from its trajectory.  -2 = a Vehicle hazard whose pose cannot be re-evaluated (it is itself a controlled /
 * caller-run agent): left unclassified.  Values <= -1 other than -2 never leave sg_read_metrics. */
typedef struct {
    double t;
    int32_t scenario, other;
    int32_t type;
    int32_t reserved;
} sg_event;

typedef struct sg_handle sg_handle;

int sg_version(void);
const char *sg_last_error(const sg_handle *h); /* valid until the next call on h; h may be NULL for create errors */

/* ScenarioGym(...) */
int sg_create(const sg_config *cfg, sg_handle **out);
int sg_destroy(sg_handle *h);

/* ScenarioGym.set_scenario -> State(...) + create_agents (scenario_gym.py:157-211): copies the
 * scenarios to HBM, builds the BatchReplayEntity union knot grids + stage-1 resample on device
 * (entity/batch.py:83-109), then resets (sg_reset). */
int sg_upload(sg_handle *h, const sg_scenarios *sc);

/* Page-locked host memory for the arrays handed to sg_upload (the knots above all: 1.6 GB for 4096 x 64 x 128).  The copy
 * engine reads such memory directly at the PCIe rate; from ordinary (pageable) memory the runtime first copies every piece
 * into a staging buffer on a CPU core, beside the host threads of sg_upload.  Ordinary memory keeps working.  No reference
 * counterpart (the reference never leaves the host).  device: the GPU the memory is registered with. */
int sg_host_alloc(int32_t device, uint64_t bytes, void **out);
int sg_host_free(void *p);

/* SocialForce(params) shared by every pedestrian agent of the handle; call before sg_upload (defaults otherwise) */
int sg_set_social_force(sg_handle *h, const sg_social_force *params);

/* Per-agent behaviour models.  The reference gives every PedestrianAgent its own behaviour object with its own parameters
 * (pedestrian/agent.py:18-41 `behaviour`, social_force.py:33-42, random_walk.py:22-31): a scenario may mix SocialForce
 * pedestrians of different parameter sets with RandomWalk pedestrians.  `models[n_models]` are the distinct (behaviour,
 * parameters, noise std) combinations of the batch, `model_of[n_scenarios * n_entities]` the model of every entity slot (read
 * for SG_KIND_AGENT_PEDESTRIAN slots only; others: any value in range, or -1).  Call before sg_upload (the batch's kernels
 * are chosen there).  One model: the same as sg_set_social_force + sg_set_ped_behaviour + the std of sg_set_ped_noise.
 * Several: every pedestrian steps under its own model (the force on a pedestrian is computed with ITS parameters from its
 * neighbours' states, social_force.py:44-114); the all-pedestrian crowd kernels, which hold one parameter set, stand back
 * for the general pedestrian variant.  The noise MODE (off / stream / device, sg_set_ped_noise) stays one per handle: the
 * reference draws every agent's two variates from the one global generator, in agent order, whatever its model.
 * SG_ERR_INVALID: more than SG_MAX_PED_MODELS models, an index out of range (a refused call leaves the handle's models as
 * they were). */
#define SG_MAX_PED_MODELS 16
typedef struct {
    int32_t behaviour;       /* SG_PED_SOCIAL_FORCE / SG_PED_RANDOM_WALK */
    int32_t reserved;
    sg_social_force params;
    double std_lon, std_lat; /* social_force.py:106-108 / random_walk.py:37-43 (used when the handle's noise mode is not off) */
} sg_ped_model;
int sg_set_ped_models(sg_handle *h, int32_t n_models, const sg_ped_model *models, const int32_t *model_of);

/* The random fluctuations of SocialForce._step (pedestrian/social_force.py:106-114): every pedestrian that is still
 * walking adds np.random.normal(bias_lon, std_lon) to its speed and np.random.normal(bias_lat, std_lat) to its heading, in
 * agent (entity) order, from numpy's global legacy generator: loc + scale * z.
 *   SG_NOISE_OFF     std = 0.
 *   SG_NOISE_STREAM  parity runs.  normals: HOST [n_scenarios][per_scenario] standard normal variates, copied by the call;
 *                    scenario r consumes row r in order, two per walking pedestrian per step -- with row r =
 *                    np.random.RandomState(k_r).standard_normal(n) the scenario reproduces the reference's rollout after
 *                    np.random.seed(k_r).  A reset rewinds the rows of the scenarios it resets.  A scenario that runs out of
 *                    variates makes sg_read_metrics fail with SG_ERR_CAPACITY (its later draws were taken as 0).
 *   SG_NOISE_DEVICE  timing / production runs: a counter-based generator on the device -- Philox4x32-10 keyed by
 *                    (seed, scenario) at counter (entity, step), Box-Muller in fp64 -- the same distribution, its own
 *                    stream, no state, no host traffic.  normals / per_scenario are ignored.
 * May be called before or after sg_upload; stays in force until the next call. */
#define SG_NOISE_OFF 0
#define SG_NOISE_STREAM 1
#define SG_NOISE_DEVICE 2
int sg_set_ped_noise(sg_handle *h, int32_t mode, double std_lon, double std_lat, const double *normals, int64_t per_scenario,
                     uint64_t seed);

/* The behaviour model of the handle's pedestrian agents (PedestrianAgent(..., behaviour=...), pedestrian/agent.py:23):
 *   SG_PED_SOCIAL_FORCE  SocialForce (pedestrian/social_force.py:33-222), the default;
 *   SG_PED_RANDOM_WALK   RandomWalk (pedestrian/random_walk.py:22-44): speed = np.random.normal(speed_desired + bias_lon,
 *                        std_lon), heading = np.random.normal(atan2(goal - position) + bias_lat, std_lat) -- no neighbours,
 *                        no speed limit other than the controller's max_speed, PedestrianAgent.force stays (0, 0).  bias_* from
 *                        sg_set_social_force, the variates and std_* from sg_set_ped_noise (two per walking pedestrian
 *                        and step, speed first, as SocialForce draws them).
 * Call before sg_upload (SG_ERR_STATE afterwards: the kernels of a batch are chosen there). */
#define SG_PED_SOCIAL_FORCE 0
#define SG_PED_RANDOM_WALK 1
int sg_set_ped_behaviour(sg_handle *h, int32_t behaviour);

/* ScenarioGym.reset_scenario -> State.reset(t0), Controller.reset, Metric.reset (scenario_gym.py:217-225) */
int sg_reset(sg_handle *h);

/* The same for the scenarios with mask[r] != 0 only (HOST [n_scenarios]): one environment of a vector of environments
 * starts a new episode (`Env.reset` of integrations/openaigym.py:128-169) while the others keep their state. */
int sg_reset_scenarios(sg_handle *h, const uint8_t *mask);

/* sg_reset_scenarios with a DEVICE mask d_mask [n_scenarios], for a caller whose done flags never leave the device: the same
 * launches -- every kernel family, scenarios of more than 512 entities and sg_set_rss on included -- queued on sg_stream(h) and
 * NOT waited for; the mask is read in stream order and must stay as it is until the reset has run.  (sg_reset_scenarios is: copy
 * the mask to the device, this, wait.)  Both start the episode accounting of sg_tick_drivers anew for the masked scenarios and
 * their drivers, and for nobody else.  SG_ERR_INVALID: d_mask NULL.  SG_ERR_STATE before sg_upload. */
int sg_reset_scenarios_device(sg_handle *h, const uint8_t *d_mask);

/* TERMINAL_CONDITIONS (state/state.py:397-408) evaluated on the current state of every scenario, all four of them
 * whatever the handle's terminal_mask: flags[r] = SG_TERM_* bits (EGO_OFF_ROAD against the networks of
 * sg_set_road_networks; none set = empty surfaces = off the road).  This is what the reward of the reference's RL agent
 * asks of a done state (integrations/openaigym.py:300-310).  out: HOST [n_scenarios] or NULL; d_out: if not NULL receives
 * a DEVICE pointer to the same flags (owned by the handle, rewritten by the next call, stream-ordered, not synchronised
 * unless `out` is given). */
int sg_terminal_flags(sg_handle *h, uint32_t *out, const uint32_t **d_out);

/* gym.timestep = x between steps (tests/test_scenario_gym.py:37-39) */
int sg_set_timestep(sg_handle *h, double timestep);

/* n x ScenarioGym.step() on every scenario, done or not (scenario_gym.py:227-254).
 * actions: HOST [n_steps][R][2] (accel, steer) for SG_KIND_AGENT_VEHICLE slots or NULL;
 * actions_device != 0 means `actions` is a DEVICE pointer of the same shape. */
int sg_step(sg_handle *h, int32_t n_steps, const double *actions, int32_t actions_device);

/* Poses returned by the caller's own agents (Agent.step(state) -> Controller.step(state, action), agent.py:52-57,
 * controller.py:30-42) for the SG_KIND_AGENT_EXTERNAL slots, consumed by every following sg_step until replaced.
 * poses: HOST [R*E][6], entity index scenario*E + slot; rows of other slots are ignored; x = NaN means the agent
 * returned None (the entity vanishes, or keeps its pose under `persist`; scenario_gym.py:233-239).  An agent that is not
 * present yet spawns at its trajectory start like every other agent (:240-244).  sg_rollout refuses batches with such
 * slots (SG_ERR_STATE): they have to be driven tick by tick. */
int sg_set_external_poses(sg_handle *h, const double *poses);

/* Per-entity vehicle actions: the drivers.  The reference gives any number of entities of one scenario an agent with a
 * VehicleController (controller.py:57-140, create_agents scenario_gym.py:188-211); sg_step's actions are one pair per scenario.
 * A driver is an SG_KIND_AGENT_EXTERNAL slot whose pose the DEVICE produces: sg_step_drivers runs VehicleController._step for it
 * from its own (accel, steer) and puts the result where sg_set_external_poses would have put it.  Driver k is entity slot slot[k]
 * of scenario scenario[k]; its controller parameters are the slot's row of sg_scenarios.ctrl (SG_C_MAX_STEER, SG_C_MAX_ACCEL,
 * SG_C_MAX_SPEED, SG_C_ALLOW_REVERSE), its wheel base the slot's bounding-box length, as for SG_KIND_AGENT_VEHICLE.
 * HOST arrays [n], copied once into a device list the handle owns; the order is the caller's and is the order of the actions.
 * n == 0 clears the list.  The list holds until it is replaced, cleared or sg_upload (which forgets it, as it forgets the
 * observers); sg_reset / sg_reset_scenarios / sg_step keep it.  SG_ERR_STATE before sg_upload.  SG_ERR_INVALID: n < 0, a NULL
 * array with n > 0, a scenario outside [0, n_scenarios), a slot outside [0, n_entities), a slot whose kind is not
 * SG_KIND_AGENT_EXTERNAL, a (scenario, slot) pair listed twice.  A refused call leaves the previous list in place.  Setting a
 * list waits for the work queued on sg_stream(h) first. */
int sg_set_drivers(sg_handle *h, int64_t n, const int32_t *scenario, const int32_t *slot);

/* n_steps x ScenarioGym.step() on every scenario, done or not, with the drivers' controllers run on the device.
 * actions: [n_steps][n_drivers][2] (accel, steer) in list order, HOST (copied into a buffer of the handle; the caller's buffer is
 * free on return) or, with actions_device != 0, a DEVICE pointer of the same shape; NULL: (0, 0) for every driver.  Nothing
 * beyond n_steps * n_drivers * 2 doubles is read.  For each step k, in this order on sg_stream(h):
 *   1. one lane per driver d = (r, slot), (a, s) = actions[k][d], t = sg_scenario_state.t of r, next_t = t + timestep,
 *      dt = next_t - t (the clock arithmetic of the step itself).
 *      The slot is not in State.poses (SG_F_PRESENT == 0): its external-pose row becomes NaN and its controller speed stays; the
 *      step spawns it at its trajectory start like every other agent (scenario_gym.py:240-244).
 *      Otherwise, with pose = its SG_F_POSE rows, speed = its SG_F_CTRL + 0 cell, l = its box length, (sin_h, cos_h) of pose[3]
 *      and the parameters of its ctrl row -- VehicleController._step, plain fp64, nothing fused:
 *        a = min(max(a, -max_accel), max_accel);  s = min(max(s, -max_steer), max_steer)
 *        x += (speed * cos_h) * dt;  y += (speed * sin_h) * dt;  h += (speed * tan(s) / l) * dt;  z, pitch, roll stay
 *        speed = speed + a * dt;  allow_reverse == 0: speed = max(0, speed);  max_speed not NaN: speed = min(max_speed, speed)
 *      the pose goes to the slot's external-pose row, the speed back to SG_F_CTRL + 0.  The same function, bit for bit, as an
 *      SG_KIND_AGENT_VEHICLE lane steps with under sg_step.  The resets write `present ? |velocity at t0| : 0` into that cell for
 *      every kind (Controller.reset, controller.py:100-103), so sg_reset / sg_reset_scenarios restart a driver's speed.
 *   2. the step of sg_step(h, 1, NULL, 0): forced, the RSS callback as sg_set_rss has it, whatever kernel family the batch takes
 *      (scenarios of more than 512 entities included).  It consumes the drivers' rows as it consumes those of
 *      sg_set_external_poses; SG_KIND_AGENT_VEHICLE slots of the batch get (0, 0); SG_KIND_AGENT_EXTERNAL slots that are not
 *      drivers keep the pose sg_set_external_poses gave them.
 * The call waits for the stream once, at its end, as sg_step does.  A driver that is the hazard of an ego collision event is
 * reported like every caller-run agent (sg_event.type -2: unclassified).  SG_ERR_STATE before sg_upload or without a driver list;
 * SG_ERR_INVALID: n_steps < 1.  One short launch ahead of every step; not part of the sg_tick graph (sg_tick and sg_rollout
 * keep refusing batches with SG_KIND_AGENT_EXTERNAL slots). */
int sg_step_drivers(sg_handle *h, int32_t n_steps, const double *actions, int32_t actions_device);

/* The built-in driver policy: traffic that reacts.  A listed driver follows a path (a polyline) with a Stanley-style steering law
 * and takes its acceleration from the Intelligent Driver Model (IDM) against the nearest box in a corridor ahead of it -- straight
 * in its heading frame, or, per driver (SG_DP_CORRIDOR), bent along its path -- and against the end of its path.  The reference has no such agent (its agents are replay, PID, pedestrian or caller-run); the
 * device evaluates the policy on the current state, so reactive traffic runs for any number of steps with no host in the loop.
 * Plain fp64, IEEE division and square root, nothing fused.
 * Policy driver j is driver driver[j] of the list of sg_set_drivers, slot so of scenario r, with the parameter row params[j]
 * (SG_DP_*) and the path pts[pt_off[j] .. pt_off[j + 1]), in driving order, used as given.  The path's segments a -> b are the rows
 * sg_set_lanes builds: e = b - a, L2 = ex*ex + ey*ey, len = sqrt(L2), cum = the sequential fp64 sum of the lens before it;
 * total = cum + len of the last segment.  A path of fewer than two points has no segments.
 * The driver has pose (x, y, h), (s, c) = sin, cos of h, v = its SG_F_CTRL + 0 cell (the controller speed of sg_step_drivers), box
 * (Wo, Lo, cxo, cyo) and front = cxo + 0.5*Lo.  A driver that is NOT in State.poses gets actions (+0.0, +0.0), info -1, -1 and feat
 * +0.0; sg_step_drivers_policy then does with it what sg_step_drivers does.  Otherwise:
 *   the path term: over the segments i of its path, (d2, dx, dy, t) by the point-to-segment rule of sg_lane_observation; a d2 that
 *   is not finite is skipped; the best segment g is the smallest (d2, i).  With it:
 *     (ux, uy) = (ex/len, ey/len), or (0, 0) when len == 0;   off = ux*dy - uy*dx
 *     se = s*ux - c*uy,  ce = c*ux + s*uy;   ce < 0 (facing against the path): se = (se >= 0 ? 1.0 : -1.0)
 *     s0 = cum + t*len,  rem = total - s0
 *     steer = -(K_PSI*se + (K_E*off) / (K_SOFT + fabs(v)))          (not clamped: VehicleController._step clamps it)
 *   With no segment: steer = +0.0, off = se = s0 = +0.0, rem = +inf.
 *   the lead: every OTHER slot e of r that is in State.poses (the presence rule of sg_nearest_entities), with pose (xe, ye, he),
 *   (sn, cn) = sin, cos of he and box (We, Le, cxe, cye):
 *     qx = xe + (cxe*cn - cye*sn),  qy = ye + (cxe*sn + cye*cn);   dx = qx - x,  dy = qy - y
 *     lon = dx*c + dy*s,  lat = dy*c - dx*s;   cr = cn*c + sn*s,  sr = sn*c - cn*s
 *     hl = 0.5*(fabs(Le*cr) + fabs(We*sr)),  hw = 0.5*(fabs(Le*sr) + fabs(We*cr));   gap = (lon - hl) - front
 *   e is a candidate iff  lat - hw <= (cyo + 0.5*Wo) + HALF  and  lat + hw >= (cyo - 0.5*Wo) - HALF  and  lon + hl > front  and
 *   gap <= REACH (inclusive); a NaN anywhere fails.  The lead is the smallest (gap, slot), the gaps compared as fp64 values (a gap
 *   may be negative; ties, -0.0 against +0.0 included, go to the lower slot);  dv = v - (vxe*c + vye*s).  With no lead: gap = +inf,
 *   dv = +0.0.  The corridor is straight, in the driver's heading frame: this is the rule of CORRIDOR == 0.
 *   the lead with CORRIDOR == 1, the corridor along the path (a driver with no best segment g -- a path of fewer than two points, or
 *   no finite distance -- uses the straight rule above): the path has n segments; front, left = (cyo + 0.5*Wo) + HALF and
 *   right = (cyo - 0.5*Wo) - HALF as above.  The window is the segments i with g <= i < n and cum_i <= (s0 + front) + REACH (cum never
 *   decreases: a contiguous range, which may be empty -- then there is no lead).  For every OTHER slot e of r that is in State.poses,
 *   with (qx, qy) and (sn, cn) as above: over the window (d2, dx, dy, t) by the point-to-segment rule at (qx, qy), a d2 that is not
 *   finite skipped, the best segment k the smallest (d2, i); with no k, or len_k == 0, e is no candidate.  Otherwise, with
 *   (ux, uy) = (ex_k/len_k, ey_k/len_k) and (dx, dy, t) of k:
 *     offe = ux*dy - uy*dx,  ce = cn*ux + sn*uy,  sne = sn*ux - cn*uy,  se = cum_k + t*len_k,  res = ux*dx + uy*dy
 *     hl = 0.5*(fabs(Le*ce) + fabs(We*sne)),  hw = 0.5*(fabs(Le*sne) + fabs(We*ce))
 *     lon = se - s0,  lat = offe - off;   gap = (lon - hl) - front
 *   e is a candidate iff  lat - hw <= left  and  lat + hw >= right  and  lon + hl > front  and  gap <= REACH  and  fabs(res) <= hl; a
 *   NaN anywhere fails.  (res: how far the box centre lies beyond the end of its segment, along it.  At an interior projection it is
 *   rounding noise; the test keeps out a box beyond the end of the window or of the path, or far out in the wedge of a sharp
 *   corner, whose arclength would be that of the corner.)  The lead is the smallest (gap, slot) as above;
 *   dv = v - (vxe*ux + vye*uy) with the direction of the lead's segment k.  With no lead: gap = +inf, dv = +0.0.  info[1] stays g.
 *   the acceleration: vr = v / V0, free = 1.0 - (vr*vr)*(vr*vr), root = 2.0*sqrt(A*B), and
 *     idm(g, d):  q = v*T + (v*d)/root;  ss = S0 + (q > 0 ? q : 0.0);  gg = g > GAP_MIN ? g : GAP_MIN;  rr = ss/gg;
 *                 idm = A*(free - rr*rr)
 *     acc = lead ? idm(gap, dv) : A*free;   with a segment: ae = idm(rem, v), acc = ae < acc ? ae : acc
 *   (ae: the end of the path as a standing obstacle).  actions = (acc, steer).
 * sg_set_driver_policy: HOST arrays, copied by the call into buffers the handle owns; NULL or m == 0 clears the policy.  The call
 * waits for the work queued on sg_stream(h) first, as sg_set_drivers does.  SG_ERR_STATE before sg_upload or with no driver list.
 * SG_ERR_INVALID: m < 0; a NULL array that is needed; a driver index outside [0, n_drivers) or not strictly ascending; pt_off not
 * starting at 0 or not monotone; a parameter that is NaN; V0, A, B, K_SOFT or GAP_MIN not > 0 or infinite; T, S0, HALF or REACH
 * < 0 (REACH alone may be +inf, T, S0 and HALF may not); K_PSI or K_E infinite; CORRIDOR neither 0.0 (straight) nor 1.0 (along the path); a NaN in pts.  A refused call leaves the previous
 * policy in place.  sg_set_drivers forgets the policy, whether it replaces or clears the list, and so does sg_upload; sg_reset /
 * sg_reset_scenarios / sg_step / sg_step_drivers keep it, and sg_step_drivers never reads it. */
enum { SG_DP_V0, SG_DP_T, SG_DP_S0, SG_DP_A, SG_DP_B, SG_DP_HALF, SG_DP_REACH,
       SG_DP_K_PSI, SG_DP_K_E, SG_DP_K_SOFT, SG_DP_GAP_MIN, SG_DP_CORRIDOR, SG_DP_NPARAM = 12 };
#define SG_DP_NINFO 2
#define SG_DP_NFEAT 6
typedef struct sg_driver_policy {
    int64_t m;              /* policy-run drivers */
    const int64_t *driver;  /* [m] positions in the list of sg_set_drivers, strictly ascending */
    const double *params;   /* [m][SG_DP_NPARAM] */
    const int64_t *pt_off;  /* [m + 1] ranges of pts, starting at 0, monotone */
    const double *pts;      /* [n_pts][2] x, y: the path of each, in driving order, used as given */
} sg_driver_policy;
int sg_set_driver_policy(sg_handle *h, const sg_driver_policy *pol);

/* The policy evaluated on the current state, for the m policy drivers in their order: actions [m][2] (acc, steer), required;
 * info [m][SG_DP_NINFO]: the lead's slot and the best segment's index within its path, -1 when none, may be NULL; feat
 * [m][SG_DP_NFEAT]: gap, dv, off, se, s0, rem, may be NULL.  Every byte of the arrays given is written.  HOST (outputs_device == 0,
 * synchronous, through a scratch of the handle) or DEVICE (queued on sg_stream(h), not waited for), as in sg_entity_status, and a
 * persistent rollout launch that gave up is reported as there.  With no policy set: SG_OK, nothing is written (actions may be NULL
 * then).  SG_ERR_INVALID: actions NULL.  SG_ERR_STATE before sg_upload.  One wavefront per policy driver: lane = path segment, then
 * lane = entity over the scenario's slots in blocks of 64; any scenario width; with CORRIDOR == 1 every lane walks the window of the
 * driver's path for its entity, so the time of such a driver grows with the segments inside REACH, not with the path.  One launch;
 * two when the policy holds drivers of both modes (the rows of either mode go to a kernel of their own, so the straight rows do not
 * carry the registers of the others).  Not part of the sg_tick graph. */
int sg_driver_policy_actions(sg_handle *h, double *actions, int32_t *info, double *feat, int32_t outputs_device);

/* sg_step_drivers with the policy in the loop: the same actions [n_steps][n_drivers][2] (HOST, DEVICE or NULL), the same order on
 * the stream, the same single wait at the end.  For each step k the action rows of the policy drivers are replaced by the policy
 * evaluated on the state before that step, ahead of the drivers' controller step; the rows of the other drivers pass through
 * untouched.  The replacement happens in a buffer of the handle: a caller's device buffer is never written.  The result is that of
 *   sg_driver_policy_actions; merge its rows into actions[k]; sg_step_drivers(h, 1, merged, ...)
 * run n_steps times, bit for bit on everything a caller can read.  One short launch more per step than sg_step_drivers.
 * SG_ERR_STATE before sg_upload, without a driver list or without a policy; SG_ERR_INVALID: n_steps < 1. */
int sg_step_drivers_policy(sg_handle *h, int32_t n_steps, const double *actions, int32_t actions_device);

/* One tick of a multi-agent environment, entirely in stream order: the step of the drivers, the terminal conditions, the status
 * (and, for a progress reward, the route observation) of every driver, reward, done, progress and episode statistics per scenario
 * and per driver, and the auto-reset of the scenarios that finished.  What a vector environment otherwise does in five to eight
 * synchronous calls with host arithmetic in between (scenario_gym_amd/vector_env.py, _step_drivers).  Nothing returns to the host.
 *
 * The rules -- with the defaults r_step = 0.01, r_bad = -1, bad_env_flags = SG_TERM_EGO_OFF_ROAD | SG_TERM_EGO_COLLISION,
 * bad_driver_flags = SG_ST_OFF_ROAD | SG_ST_COLLISION the reward of the reference's RLAgent (integrations/openaigym.py:300-310)
 * asked per scenario and per driver: */
typedef struct sg_episode_rules {
    uint32_t terminal_mask;    /* SG_TERM_* bits that end a scenario's episode */
    uint32_t bad_env_flags;    /* SG_TERM_* bits that make the reward of a finished scenario r_bad */
    uint32_t bad_driver_flags; /* SG_ST_* bits that make a driver's base reward r_bad and end its episode */
    int32_t auto_reset;        /* != 0: the scenarios that finished are reset behind the tick (reset_mask = env_done) */
    double r_step, r_bad;      /* finite */
    double w_progress;         /* finite; the weight of the arclength a driver gained along its route of sg_set_routes; 0: no route
                                  observation is launched */
} sg_episode_rules;

/* What a tick leaves behind: const DEVICE pointers into buffers the handle owns, written in stream order by the tick that returned
 * them (sg_synchronize, or work queued on sg_stream(h), sees them complete) and valid until the next sg_tick_drivers,
 * sg_set_drivers or sg_upload.  n_drv = the drivers of sg_set_drivers, rows in list order, policy-run drivers included.  The
 * status and route rows are those of the stepped state, BEFORE the auto-reset replaced it. */
typedef struct sg_episode_view {
    const uint32_t *term_flags;     /* [n_scenarios] sg_terminal_flags of the stepped state */
    const uint8_t *env_done;        /* [n_scenarios] */
    const double *env_reward;       /* [n_scenarios] */
    const uint8_t *reset_mask;      /* [n_scenarios] the scenarios the tick reset */
    const int32_t *ep_length;       /* [n_scenarios] ticks of the scenario's episode, this one included */
    const uint32_t *drv_flags;      /* [n_drv] sg_entity_status of every driver: flags, */
    const int32_t *drv_info;        /* [n_drv][SG_ST_NINFO] info */
    const double *drv_feat;         /* [n_drv][SG_ST_NFEAT] and feat */
    const double *drv_route;        /* [n_drv][SG_RT_NFEAT] sg_route_observation with n_ahead = 0; NULL when w_progress == 0 */
    const int32_t *drv_route_info;  /* [n_drv][SG_RT_NINFO]; NULL when w_progress == 0 */
    const double *drv_progress;     /* [n_drv] */
    const double *drv_reward;       /* [n_drv] */
    const double *ep_return;        /* [n_drv] the sum of the driver's rewards over its scenario's episode, this tick included */
    const uint8_t *drv_done;        /* [n_drv] */
} sg_episode_view;

/* actions: [n_drv][2] (acceleration, steering) in list order, HOST (actions_device == 0), DEVICE, or NULL for (0, 0); the rows of
 * policy drivers are replaced by the policy's.  Queued on sg_stream(h), in this order:
 *   1. with a policy set (sg_set_driver_policy): driver_policy_kernel into the merged action buffer of the handle
 *   2. drive_kernel: the drivers' controller step
 *   3. one forced step of the batch -- 1 to 3 are sg_step_drivers / sg_step_drivers_policy with n_steps = 1 without their wait
 *   4. terminal_flags
 *   5. entity_status on the DRIVER list (the observer list of sg_set_observers is neither read nor touched)
 *   6. with w_progress != 0: route_observation on the driver list, n_ahead = 0
 *   7. episode_kernel (csrc/sgym_episode.hpp), one lane per index i < max(n_scenarios, n_drv), plain unfused fp64:
 *      scenario r, f = term_flags[r]:
 *        env_done[r] = (f & terminal_mask) != 0;  env_reward[r] = env_done[r] && (f & bad_env_flags) ? r_bad : r_step
 *        reset_mask[r] = auto_reset && env_done[r]
 *        ep_length[r] = ++length[r] (the handle's counter), which is then zeroed when reset_mask[r]
 *      driver d of scenario r:
 *        bad = (drv_flags[d] & bad_driver_flags) != 0;  base = bad ? r_bad : r_step
 *        w_progress == 0: drv_progress[d] = +0.0, drv_reward[d] = base, and the route memory below is left alone
 *        otherwise: on = drv_route_info[d][0] >= 0, s0 = drv_route[d][8];
 *          drv_progress[d] = on && prev_ok[d] ? s0 - prev_s[d] : +0.0;  drv_reward[d] = base + w_progress * drv_progress[d] (the
 *          product rounded, then the sum);  prev_s[d] = s0;  prev_ok[d] = on && !reset_mask[r]
 *        drv_done[d] = bad || env_done[r]
 *        ep_return[d] = (return[d] += drv_reward[d]) (the handle's accumulator), which is then zeroed when reset_mask[r]
 *   8. with auto_reset: sg_reset_scenarios_device on reset_mask
 * prev_s, prev_ok, return and length live on the handle.  sg_reset, sg_upload, sg_set_drivers and sg_set_routes zero them for
 * everybody, sg_reset_scenarios[_device] for the masked scenarios and their drivers; sg_step* leave them alone.  So the first tick
 * of an episode has progress 0.
 * The call never waits for the stream, except that HOST actions are copied before it returns (the caller's array is free then);
 * the first call after the driver list changed allocates.  It is a sequence of plain stream-ordered launches, not a captured
 * graph: it may be queued any number of times without a wait in between, and must not be called while sg_stream(h) is
 * capturing.  A persistent rollout launch that gave up is reported as the DEVICE-output observation calls report it (what is
 * known so far).  Every byte of every array of the view is written by every tick.
 * SG_ERR_STATE before sg_upload or without a driver list; SG_ERR_INVALID: rules or out NULL, r_step, r_bad or w_progress NaN or
 * infinite.  A refused call queues nothing and leaves state, accounting and *out as they were. */
int sg_tick_drivers(sg_handle *h, const double *actions, int32_t actions_device, const sg_episode_rules *rules, sg_episode_view *out);

/* Device snapshots: go back to a saved state, every scenario or the masked ones.  The reference has no counterpart (a State is
 * deep-copied by hand there); planners over the simulator (save, roll candidates, go back), resets to saved situations and
 * counterfactuals need it, and with sg_tick / sg_tick_drivers the state never leaves the device.
 * STATE is everything a later call reads of what an earlier call wrote: the entity blocks and sg_scenario_state (noise_pos, the
 * position in a scenario's noise stream, included), the collision events with the poses kept beside them, the pose record, the poses
 * of sg_set_external_poses (a driver's pose included), the RSSDistances records when they exist, CollisionMetric.last_timestep and
 * the twin table of scenarios of more than 512 entities, and the episode accounting of sg_tick_drivers (previous arclength, return,
 * length).  SETTINGS are not state and are not saved: the timestep, the pedestrian models and noise settings, road networks, lanes,
 * observers, drivers, policy, routes, tuning.
 * What "restored" means: after sg_snapshot_restore(h, s, mask, ..), for every scenario r with mask[r] != 0, every later call -- a
 * step by any entry point and kernel family, every read and observation -- returns for r byte for byte what it would have returned
 * had it been made right after the sg_snapshot_save (or the create) that last wrote r's rows of s, whatever happened on the handle in
 * between; scenarios with mask[r] == 0 are untouched, on the handle and in the snapshot.
 *
 * sg_snapshot_create: device room for one copy of every state array, then a save of every scenario -- a snapshot never holds an
 * unsaved row, so a masked restore is always defined.  It allocates and may therefore wait for the device.  Arrays the handle makes
 * on first use come into being here as that use would make them: the RSSDistances records when sg_set_rss is on (as sg_reset makes
 * them: the callback runs once on the current state), the episode buffer when a driver list is set, the scratch of scenarios of more
 * than 512 entities.  Any number of snapshots per handle, independent of each other; the handle owns them, sg_snapshot_destroy (which
 * waits for sg_stream(h)) or sg_destroy frees them.  sg_snapshot_bytes: the device bytes of one.
 *
 * sg_snapshot_save copies the rows of the masked scenarios from the handle into the snapshot, sg_snapshot_restore copies them back.
 * mask: [n_scenarios] bytes, NULL = every scenario; mask_device == 0: a HOST array, copied before the call returns (the caller's
 * array is free then); else a DEVICE pointer read in stream order, which must stay as it is until the copy has run (as
 * sg_reset_scenarios_device reads its mask).  The drivers of a scenario go with their scenario, as in sg_reset_scenarios.
 * Order: both are queued on sg_stream(h) behind everything earlier calls queued on either stream of the handle, and never wait for
 * the device: they may stand back to back with sg_step*, sg_tick_drivers, sg_rollout_async and the observation calls.  One kernel
 * launch per call (plus the copy of a HOST mask).  Not to be called while sg_stream(h) is capturing.  The copy is in place, no
 * address moves: a captured sg_tick graph and the pointers of sg_state_view / sg_episode_view stay valid across a restore.
 * Episode accounting that is due to start anew (after sg_reset, sg_set_routes: the next tick would zero it) is zeroed first, by save
 * and by restore, which a caller cannot tell from the tick doing it.
 * SG_ERR_INVALID: h, s or out NULL, or a snapshot that is not one of this handle's.  SG_ERR_STATE: before sg_upload; the batch
 * (sg_upload), the driver list (sg_set_drivers) or sg_set_rss changed since the snapshot was created (the message names which; the
 * snapshot can then only be destroyed).  A persistent rollout launch that gave up is sticky and reported with its own code and
 * message, as sg_tick_drivers reports it.  A refused call queues nothing and changes nothing. */
typedef struct sg_snapshot sg_snapshot; /* opaque, owned by the handle it was created on */
int sg_snapshot_create(sg_handle *h, sg_snapshot **out);
int sg_snapshot_save(sg_handle *h, sg_snapshot *s, const uint8_t *mask, int32_t mask_device);
int sg_snapshot_restore(sg_handle *h, sg_snapshot *s, const uint8_t *mask, int32_t mask_device);
int sg_snapshot_bytes(sg_handle *h, const sg_snapshot *s, uint64_t *bytes);
int sg_snapshot_destroy(sg_handle *h, sg_snapshot *s);

/* ScenarioGym.rollout(): reset, then step each scenario while it is not done, at most max_steps
 * (scenario_gym.py:256-267).  The time loop runs inside the kernels: one launch for short runs; long runs of batches with
 * PID / vehicle agents as ONE persistent launch that carries the controller pre-pass (sg_schedule_info), else one launch per
 * chunk of steps.  Scenarios of more than 512 entities step through four launches per step; the host only enqueues there
 * too (every 64 steps a kernel reports into page-locked memory how many scenarios still run, and the call stops enqueuing
 * once an earlier report says none: the steps enqueued meanwhile are no-ops). */
int sg_rollout(sg_handle *h, int32_t max_steps);
/* Same without the reset and without waiting: enqueue on the handle's stream (bench timing) */
int sg_rollout_async(sg_handle *h, int32_t max_steps, int32_t do_reset);
int sg_synchronize(sg_handle *h);
void *sg_stream(sg_handle *h); /* hipStream_t */

int sg_state_view_get(sg_handle *h, sg_state_view *out);

/* FutureCollisionDetector._step (sensor/common.py:59-106) for the ego of every scenario at its current State.t:
 * out[r] = 1 iff, at one of the n_samples times np.linspace(t, t + horizon, n_samples), the ego's box at
 * trajectory.position_at_t(t_j) overlaps another entity's box at that entity's own position_at_t(t_j) (reference
 * defaults: horizon 5.0, 10 samples).  out: HOST [R]. */
int sg_future_collision(sg_handle *h, double horizon, int32_t n_samples, uint8_t *out);

/* RasterizedMapSensor "entity" layer (sensor/map.py:120-192) for the ego of every scenario at the current state:
 * out[r][i][j] = 1 iff the point (linspace(-width/2, width/2, nw)[j], linspace(-height/2, height/2, nh)[i]) of the ego's
 * frame (rotated by heading + pi/2) lies strictly inside the bounding box of a present entity, the ego included;
 * all zeros for a scenario whose ego is absent.  The reference sensor has nw == nh.  out: HOST [R][nh][nw] bytes. */
int sg_raster_entities(sg_handle *h, double width, double height, int32_t nw, int32_t nh, uint8_t *out);

/* Scenario.road_network for the uploaded batch: after sg_upload (which forgets the previous networks), before the
 * first step that needs them.  `contains(Point)` on a union (state.py:401-407, sensor/map.py:198-271) is answered as
 * shapely answers it for points that are not on a polygon's boundary: strictly inside one of the polygons of the union,
 * by the crossing number of its rings with an exact orientation sign (JTS/GEOS RayCrossingCounter); points ON a ring are
 * outside.  The library lays a uniform grid over each network (cells wholly inside / wholly outside a union answer at
 * once, the others test the polygons that cross them) -- an index only, the answers are those of the plain test. */
int sg_set_road_networks(sg_handle *h, const sg_road_networks *nets);

/* RasterizedMapSensor._step (sensor/map.py:136-149) for the ego (entities[0] of the reference's tests = the scenario's
 * ego) of every scenario: layers[k] = 0 is the "entity" layer of sg_raster_entities, otherwise ONE SG_LAYER_* bit
 * ("driveable_surface", "road", "intersection", "lane", "walkable_surface", "pavement", "crossing");
 * out[r][k][i][j] as in sg_raster_entities (the sensor's channels_first layout).  out: HOST [R][n_layers][nh][nw]. */
int sg_raster_map(sg_handle *h, double width, double height, int32_t nw, int32_t nh, int32_t n_layers,
                  const int32_t *layers, uint8_t *out);

/* The same maps left in device memory for a policy that runs on this GPU (the observation of
 * integrations/openaigym.py:280-297 without the trip through the host): *d_out = DEVICE [R][n_layers][nh][nw] bytes inside
 * the handle's observation scratch, written by kernels queued on sg_stream(h) -- not synchronised; valid until the next
 * observation call (sg_raster_*, sg_future_collision) or sg_destroy. */
int sg_raster_map_device(sg_handle *h, double width, double height, int32_t nw, int32_t nh, int32_t n_layers,
                         const int32_t *layers, const uint8_t **d_out);

/* State.get_road_info_at_entity (state/state.py:330-338) for every entity slot of the batch at its current pose: the
 * geometries x of the scenario's network with x.boundary.contains(Point(pose[:2])) -- strictly inside the polygon's exterior
 * ring and outside its holes; a point on one of its rings is not contained.  Every polygon of sg_road_networks answers for
 * itself, whatever its SG_LAYER_* bits (zero included); the answer is exact for the fp64 coordinates given.  Per slot
 * i = scenario * n_entities + slot:
 *   count[i]       how many geometries contain the entity (it may exceed cap); -1 for a slot that is not in State.poses
 *                  (padding, vanished, not spawned yet: the reference raises KeyError); 0 in a scenario without a network
 *                  (the reference returns ([], [])) and on a handle without sg_set_road_networks
 *   geoms[i][cap]  their indices in ascending order, -1 behind the last: the polygon's position within its own network
 *                  (polygon poly_off[n] is index 0 of network n).  May be NULL; `cap` is ignored then
 *   layers[i]      the OR of the SG_LAYER_* bits of ALL containing polygons, those beyond cap too.  May be NULL
 * outputs_device == 0: HOST buffers, synchronous.  Otherwise all three are DEVICE pointers; the kernel is queued on
 * sg_stream(h) behind the handle's pending work and the call does not wait (valid after sg_synchronize).
 * SG_ERR_INVALID: count NULL, cap < 0.  One lookup in the cell grid of sg_set_road_networks per entity: the cell lists the
 * polygons covering it and the polygons whose boundary crosses it, and only the latter are tested, on their edges there. */
int sg_road_info(sg_handle *h, int32_t cap, int32_t *count, int32_t *geoms, uint32_t *layers, int32_t outputs_device);

/* RoadNetwork.get_geometries_at_point (road_network/road_network.py:375-407) for n points: point k = (xy[k][0], xy[k][1])
 * against the network of scenario scenario_of_point[k].  count [n], geoms [n][cap], layers [n] as above (count is never
 * -1 here; a point with a NaN coordinate is in nothing).  HOST arrays, synchronous.  SG_ERR_INVALID: n < 0, count NULL,
 * cap < 0, xy or scenario_of_point NULL with n > 0, a scenario index outside [0, n_scenarios). */
int sg_road_info_points(sg_handle *h, int64_t n, const int32_t *scenario_of_point, const double *xy, int32_t cap, int32_t *count,
                        int32_t *geoms, uint32_t *layers);

/* The observers of the two calls below: observer k is entity slot slot[k] of scenario scenario[k] -- ANY entity of its
 * scenario, as the reference's sensors are built per entity (RasterizedMapSensor(entity, ...) sensor/map.py:136-271,
 * FutureCollisionDetector(entity, horizon) sensor/common.py:60-106; create_agent gives them to agents of non-ego entities).
 * HOST arrays [n], copied once into a device list the handle owns; duplicates are allowed and the order is the caller's.  The
 * list holds until it is replaced, cleared (n == 0) or sg_upload (which forgets it, as it forgets the road networks);
 * sg_reset / sg_step / sg_rollout keep it.  SG_ERR_STATE before sg_upload.  SG_ERR_INVALID: n < 0, a NULL array with n > 0, a
 * scenario outside [0, n_scenarios), a slot outside [0, n_entities), a slot of SG_KIND_NONE, n above 2^31 - 1 (one workgroup
 * serves one observer: the grid limit).  A refused call leaves the handle without observers.  Replacing or setting a list waits
 * for the work queued on sg_stream(h) first (a queued observation call may still read the previous list): do it between
 * episodes, not inside a pipelined step loop. */
int sg_set_observers(sg_handle *h, int64_t n, const int32_t *scenario, const int32_t *slot);

/* RasterizedMapSensor._step (sensor/map.py:136-271) for every observer, in the observer's frame (rotated by its heading +
 * pi/2): out[k][l][i][j] as sg_raster_map has it for the ego -- layers[l] = 0 the "entity" layer, otherwise ONE SG_LAYER_* bit,
 * 1..8 layers; a surface layer on a handle without networks or in a scenario without one is all zeros; an observer that is
 * not in State.poses (the reference sensor reads state.poses[entity]) gets all zeros.  For the observer (r, ego of r) the
 * bytes are those of sg_raster_map.  out: [n_observers][n_layers][nh][nw] bytes.  outputs_device == 0: HOST buffer,
 * synchronous (the maps pass through the handle's observation scratch: an observation call).  Otherwise `out` is a DEVICE
 * pointer; the kernel is queued on sg_stream(h) behind the handle's pending work and the call does not wait (valid after
 * sg_synchronize).  With no observers set: SG_OK, nothing is written.  A persistent rollout launch that gave up is reported as
 * by the other observation calls (sticky); a call that does not wait -- device outputs, no observers -- reports what is
 * known when it is made, and the give-up of a launch still in flight is reported by the next call that synchronises.  One
 * workgroup per observer computes all layers in one pass over the grid points.  Not part of the sg_tick graph. */
int sg_raster_map_observers(sg_handle *h, double width, double height, int32_t nw, int32_t nh, int32_t n_layers,
                            const int32_t *layers, uint8_t *out, int32_t outputs_device);

/* FutureCollisionDetector._step (sensor/common.py:87-106) for every observer at the current State.t of its scenario:
 * out[k] = 1 iff, at one of the n_samples times np.linspace(t, t + horizon, n_samples), the observer's box at its
 * trajectory.position_at_t(t_j) overlaps another entity's box at that entity's own position_at_t(t_j); presence is not
 * consulted and a box equal to the observer's never counts, as in sg_future_collision, whose answer the observer
 * (r, ego of r) reproduces.  out: [n_observers] bytes, HOST or DEVICE as in sg_raster_map_observers. */
int sg_future_collision_observers(sg_handle *h, double horizon, int32_t n_samples, uint8_t *out, int32_t outputs_device);

/* The vector observation: the k nearest entities around the ego of every scenario (n = n_scenarios observers), in the ego's
 * frame.  The reference has no such sensor (its State.get_entities_in_radius answers for one scenario on the host); this is
 * the policy input driving-RL code uses in place of a map image.  For observer o = slot so of scenario r with pose
 * (xo, yo, ho), velocity (vxo, vyo) and (s, c) = sin, cos of ho, every OTHER slot e of r that is in State.poses gives
 * dx = xe - xo, dy = ye - yo, d2 = dx * dx + dy * dy (plain fp64).  e is a candidate iff d2 is finite and
 * d2 <= radius * radius (inclusive; radius = +inf: every present entity).  The candidates are ordered by ascending (d2, slot)
 * -- ties in d2 go to the lower slot -- and the first k give, with (se, ce) = sin, cos of he:
 *   feat[o][j][0..7]  dx*c + dy*s (along the observer's heading), dy*c - dx*s (left positive), ce*c + se*s and se*c - ce*s
 *                     (cos, sin of the relative heading), dvx*c + dvy*s and dvy*c - dvx*s (dvx = vxe - vxo, dvy = vye - vyo),
 *                     the neighbour's box length, its box width; rows behind the last neighbour are +0.0
 *   slots[o][j]       the neighbour's slot, -1 behind the last.  May be NULL
 *   count[o]          the number of candidates within the radius (it may exceed k).  May be NULL
 * An observer that is not in State.poses gets count -1, slots -1 and features 0.0 (as sg_road_info answers for such a slot).
 * Every byte of the outputs given is written.  feat: [n][k][8] doubles, slots: [n][k], count: [n]; HOST (outputs_device == 0,
 * synchronous, through the observation scratch) or DEVICE (queued on sg_stream(h), not waited for), as in
 * sg_raster_map_observers, and a persistent rollout launch that gave up is reported as there.  SG_ERR_INVALID: k < 1, k > 32,
 * radius NaN or negative, feat NULL.  SG_ERR_STATE before sg_upload.  One wavefront per observer keeps the keys of up to 512
 * slots in registers and selects in k rounds of a cross-lane minimum; wider scenarios take one workgroup per observer.  Not
 * part of the sg_tick graph: queue it behind sg_tick with device outputs. */
int sg_nearest_entities(sg_handle *h, int32_t k, double radius, double *feat, int32_t *slots, int32_t *count, int32_t outputs_device);

/* The same for every observer of sg_set_observers (n = their number; duplicates each get their rows).  For the observer
 * (r, ego of r) the bytes are those of sg_nearest_entities for scenario r.  With no observers set: SG_OK, nothing is written
 * (feat may be NULL then). */
int sg_nearest_entities_observers(sg_handle *h, int32_t k, double radius, double *feat, int32_t *slots, int32_t *count,
                                  int32_t outputs_device);

/* The pose history: where the ego of every scenario (n = n_scenarios observers) and the k entities nearest to it were at the
 * last n_samples rows of the pose record, `stride` rows apart, in the ego's CURRENT frame -- the input of vectorised driving
 * policies and trajectory predictors.  The reference has no such sensor (its State.recorded_poses hands the whole record to
 * the host).  It reads the record a handle created with record_capacity > 0 keeps on the device: one row of poses and one time
 * per scenario at reset and behind every step, NaN in all six coordinates of an entity that is not in State.poses, L = rec_rows
 * rows of scenario r so far; every kind of reset takes L back to 1.  Nothing is stepped and nothing of the record is changed.
 * For observer o = slot so of scenario r with current pose (xo, yo, ho), (s, c) = sin, cos of ho, and t = State.t of r:
 *   subjects   subject 0 is the observer itself.  Subjects 1..k are the neighbours sg_nearest_entities_observers(k, radius)
 *              selects at the current state, by exactly its rule and in its order: the other slots of r that are in
 *              State.poses with a finite d2 <= radius * radius, ascending (d2, slot).  slots[o][i - 1] and count[o] carry the
 *              bytes that call would write.  k == 0: the observer's own history alone (slots may be NULL; count is still the
 *              number of candidates within the radius).
 *   samples    sample j in [0, n_samples) reads record row rho = L - 1 - j * stride; sample 0 is the current state.
 *   validity   sample j of subject e is valid iff rho >= 0 and the recorded x of e in row rho is not NaN.
 * With (X, Y, Hd) the recorded coordinates 0, 1 and 3 of e in row rho, (se, ce) = sin, cos of Hd, dx = X - xo, dy = Y - yo, a
 * valid sample gives
 *   feat[o][i][j][0..5]  dx*c + dy*s (along the observer's heading now), dy*c - dx*s (left positive), ce*c + se*s and
 *                        se*c - ce*s (cos, sin of the heading then relative to the observer's now), t - rec_t[rho] (the age of
 *                        the sample in seconds; +0.0 for j = 0), 1.0
 * in plain fp64, unfused, as sg_nearest_entities computes its rows.  An invalid sample is six +0.0, and so is every sample of
 * a subject row behind the last neighbour.
 * A STALE record -- rec_rows != n_steps + 1 of r: the record filled up and the scenario went on stepping, so its last row is
 * not the current state -- gives count -2, slots -1 and all features +0.0 for every observer of r: old rows are never presented
 * as recent ones.  Otherwise an observer that is not in State.poses gets count -1, slots -1 and all features +0.0, as in
 * sg_nearest_entities.
 * Every byte of the outputs given is written.  feat: [n][1 + k][n_samples][6] doubles, slots: [n][k], count: [n], may be NULL;
 * HOST (outputs_device == 0, synchronous, through the observation scratch) or DEVICE (queued on sg_stream(h), not waited for),
 * as in sg_nearest_entities, and a persistent rollout launch that gave up is reported as there.  SG_ERR_INVALID: n_samples
 * outside 1..SG_HIST_MAX_SAMPLES, stride outside 1..SG_HIST_MAX_STRIDE, k outside 0..32, radius NaN or negative, feat NULL.
 * SG_ERR_STATE: the call needs a pose record -- a handle created with record_capacity == 0 has none --, and before sg_upload.
 * The record costs record_capacity * 6 * n_scenarios * entity_stride * 8 bytes of device memory, which snapshots copy too.
 * One wavefront per observer selects as sg_nearest_entities does and walks the (subject, sample) pairs 64 at a time, subject
 * fastest; scenarios of more than 512 entities take one workgroup per observer.  Not part of the sg_tick graph: queue it
 * behind sg_tick / sg_tick_drivers with device outputs. */
#define SG_HIST_MAX_SAMPLES 64
#define SG_HIST_MAX_STRIDE (1 << 20)
int sg_pose_history(sg_handle *h, int32_t n_samples, int32_t stride, int32_t k, double radius, double *feat, int32_t *slots,
                    int32_t *count, int32_t outputs_device);

/* The same for every observer of sg_set_observers (n = their number; duplicates each get their rows).  For the observer
 * (r, ego of r) the bytes are those of sg_pose_history for scenario r.  With no observers set: SG_OK, nothing is written
 * (feat may be NULL then). */
int sg_pose_history_observers(sg_handle *h, int32_t n_samples, int32_t stride, int32_t k, double radius, double *feat,
                              int32_t *slots, int32_t *count, int32_t outputs_device);

/* The lane centre lines of the networks of sg_set_road_networks, which comes first: its net_of_scenario tells which
 * network a scenario uses.  SG_ERR_STATE before sg_upload or before sg_set_road_networks.  SG_ERR_INVALID: n_networks other
 * than that call's, offsets that do not start at 0 or are not monotone, a successor index outside its network, a NULL array
 * that is needed, 2^31 or more lanes or segments.  A refused call changes nothing.  sg_upload and sg_set_road_networks forget
 * the lanes, as sg_upload forgets the networks and the observers.  The call waits for the work queued on sg_stream(h) (a queued
 * sg_lane_observation may still read the previous lanes) and builds one device row per segment a -> b of every centre line,
 * lane by lane in point order -- a, e = b - a, L2 = ex*ex + ey*ey (unfused), len = sqrt(L2), cum = the arclength of a within
 * its lane as the sequential fp64 sum of the preceding len (0 for the first segment), b -- and per lane its segment range,
 * total = cum + len of its last segment and its successors. */
int sg_set_lanes(sg_handle *h, const sg_lanes *lanes);

#define SG_LANE_MAX_K 8      /* lanes per observer */
#define SG_LANE_MAX_AHEAD 16 /* centre-line points ahead per lane */
#define SG_LANE_MAX_HOPS 4   /* successors a look-ahead point may walk through */

/* The lane-frame vector observation of the ego of every scenario (n = n_scenarios observers): where the vehicle is relative
 * to the k nearest lanes of its scenario's network and where their centre lines go next.  The reference has no such sensor (it
 * stores Lane.center and the successor ids, road_network/objects.py, road_network.py:349-355).  Plain fp64 with IEEE division
 * and square root, no fused operation.  For an observer with pose (px, py, h) and (s, c) = sin, cos of h:
 *   projection onto segment i (a, b, e, L2 as sg_set_lanes built them) of its scenario's network: wx = px - ax, wy = py - ay,
 *     t = (wx*ex + wy*ey) / L2; the closest point (cx, cy) is a when L2 == 0 or !(t > 0) (then t counts as 0), b exactly -- the
 *     stored point, not a + e -- when t >= 1 (t counts as 1), else (ax + t*ex, ay + t*ey); dx = px - cx, dy = py - cy,
 *     d2 = dx*dx + dy*dy; a segment whose d2 is not finite is skipped
 *   a lane's key is the smallest (d2, segment index) over its segments; the lane is a candidate iff that d2 <= radius * radius
 *     (inclusive; radius = +inf: every lane that has a segment); the candidates are ordered by ascending (d2, lane index) -- two
 *     lanes that share an end point tie exactly and the lower index wins -- and the first k fill the rows
 *   feat[o][j][0 .. 5 + 2*n_ahead] for a chosen lane with best segment i, (ux, uy) = (ex/len, ey/len) or (0, 0) when len == 0:
 *     [0] ux*dy - uy*dx, the lateral offset, left of the lane direction positive; [1] c*ux + s*uy and [2] s*ux - c*uy, cos and sin
 *     of the observer's heading relative to the lane; [3] s0 = cum + t*len, the arclength along the lane; [4] total - s0;
 *     [5] sqrt(d2); then for m = 1..n_ahead the centre-line point at arclength target = s0 + (double)m * spacing, walked from
 *     the chosen lane anew for every m: while target > total of the lane, fewer than SG_LANE_MAX_HOPS hops were made and the
 *     lane has a successor with at least one segment, target -= total and the lane becomes its lowest-index such successor; if
 *     target > total still, the point is the lane's last point; else with g the last segment of the lane with cum[g] <= target
 *     and u = (target - cum[g]) / len[g] (0 when len[g] == 0) the point is b of g when u >= 1, else (ax + u*ex, ay + u*ey).
 *     With X = x - px, Y = y - py: [6 + 2(m-1)] = X*c + Y*s, [7 + 2(m-1)] = Y*c - X*s (the observer's frame)
 *   lanes[o][j]  the lane's index within its network, -1 behind the last candidate.  May be NULL
 *   count[o]     the number of candidates (it may exceed k).  May be NULL
 * Rows behind the last candidate are +0.0.  An observer that is not in State.poses gets count -1, lanes -1 and zeros; a
 * scenario without a network, or a handle without sg_set_lanes, count 0, lanes -1 and zeros.  Every byte of the outputs given
 * is written.  feat: [n][k][6 + 2*n_ahead] doubles, lanes: [n][k], count: [n]; HOST (outputs_device == 0, synchronous, through
 * the observation scratch) or DEVICE (queued on sg_stream(h), not waited for), as in sg_nearest_entities, and a persistent
 * rollout launch that gave up is reported as there.  SG_ERR_INVALID: k outside 1..SG_LANE_MAX_K, n_ahead outside
 * 0..SG_LANE_MAX_AHEAD, spacing NaN, negative or infinite, radius NaN or negative, feat NULL.  SG_ERR_STATE before sg_upload.
 * One wavefront per observer tests every segment of the network (the committed networks have at most 11,040 centre points: no
 * index) and selects in k rounds of a cross-lane minimum.  Not part of the sg_tick graph. */
int sg_lane_observation(sg_handle *h, int32_t k, int32_t n_ahead, double spacing, double radius,
                        double *feat, int32_t *lanes, int32_t *count, int32_t outputs_device);

/* The same for every observer of sg_set_observers (n = their number; duplicates each get their rows).  For the observer
 * (r, ego of r) the bytes are those of sg_lane_observation for scenario r.  With no observers set: SG_OK, nothing is written
 * (feat may be NULL then). */
int sg_lane_observation_observers(sg_handle *h, int32_t k, int32_t n_ahead, double spacing, double radius,
                                  double *feat, int32_t *lanes, int32_t *count, int32_t outputs_device);

/* The range scan (lidar): a fan of n_rays beams from the pose point of the ego of every scenario (n = n_scenarios observers),
 * each reporting the distance to the first other entity's box it meets and how fast that distance changes.  The reference
 * has no such sensor (its RasterizedMapSensor is the image-shaped equivalent); the nearest-entity rows give reference points,
 * not box surfaces, and know nothing of occlusion.  Plain fp64, IEEE division, nothing fused.
 * The observer is slot so of scenario r with pose (xo, yo, ho), velocity (vxo, vyo) and (s, c) = sin, cos of ho.  Beam b in
 * [0, n_rays) has the angle a_b = angle0 + (double)b * dangle from the observer's heading, (sb, cb) = sin, cos of a_b, and the
 * world direction ux = cb*c - sb*s, uy = sb*c + cb*s.  Every OTHER slot e of r that is in State.poses (the presence rule of
 * sg_nearest_entities), with pose (xe, ye, he), (se, ce) = sin, cos of he and box (W, L, cx, cy) = (width, length, center_x,
 * center_y), is met in its own frame -- the inverse of the rotation Entity.get_bounding_box_points applies, so the same
 * rectangle up to rounding:
 *   dx = xo - xe, dy = yo - ye;  ox = dx*ce + dy*se, oy = dy*ce - dx*se;  lx = ux*ce + uy*se, ly = uy*ce - ux*se
 *   x-slab: lo = cx - 0.5*L, hi = cx + 0.5*L against (ox, lx);  y-slab: lo = cy - 0.5*W, hi = cy + 0.5*W against (oy, ly)
 *   slab (o, l, lo, hi): l == 0: (tn, tf) = (-inf, +inf) when o >= lo && o <= hi, else (+inf, -inf); otherwise t1 = (lo - o)/l,
 *     t2 = (hi - o)/l, tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1
 *   tmin = 0; if (tnx > tmin) tmin = tnx; if (tny > tmin) tmin = tny;  tmax = tfy < tfx ? tfy : tfx
 *   e is hit iff tmin <= tmax && tmin <= max_range && tmin < +inf (inclusive; an origin inside or on a box gives 0; any NaN
 *   gives no hit)
 * The beam's hit is the smallest (tmin, slot) over the hit entities: ties in range go to the lower slot.
 *   feat[o][b][0]  the range tmin; max_range (which may be +inf) without a hit
 *   feat[o][b][1]  the range rate (vxe - vxo)*ux + (vye - vyo)*uy of the hit entity, negative when it closes along the beam;
 *                  +0.0 without a hit
 *   slots[o][b]    the hit slot, -1 without.  May be NULL
 *   hits[o]        the number of beams that hit something.  May be NULL
 * An observer that is not in State.poses gets hits -1, slots -1 and features +0.0.  Every byte of the outputs given is
 * written.  feat: [n][n_rays][2] doubles, slots: [n][n_rays], hits: [n]; HOST (outputs_device == 0, synchronous, through the
 * observation scratch) or DEVICE (queued on sg_stream(h), not waited for), as in sg_nearest_entities, and a persistent rollout
 * launch that gave up is reported as there.  SG_ERR_INVALID: n_rays outside 1..SG_SCAN_MAX_RAYS, angle0 or dangle NaN or
 * infinite, max_range NaN or negative, feat NULL.  SG_ERR_STATE before sg_upload.  A refused call writes nothing and leaves
 * the handle working.  One wavefront per observer computes what a beam needs of an entity once per observer, 64 entities at a
 * time, and runs 64 beams against them; any scenario width.  Not part of the sg_tick graph. */
#define SG_SCAN_MAX_RAYS 1024
int sg_range_scan(sg_handle *h, int32_t n_rays, double angle0, double dangle, double max_range, double *feat, int32_t *slots,
                  int32_t *hits, int32_t outputs_device);

/* The same for every observer of sg_set_observers (n = their number; duplicates each get their rows).  For the observer
 * (r, ego of r) the bytes are those of sg_range_scan for scenario r.  With no observers set: SG_OK, nothing is written
 * (feat may be NULL then). */
int sg_range_scan_observers(sg_handle *h, int32_t n_rays, double angle0, double dangle, double max_range, double *feat,
                            int32_t *slots, int32_t *hits, int32_t outputs_device);

/* The episode status of an entity: what a per-agent reward and termination need of the ego of every scenario (n = n_scenarios
 * observers) in one launch -- whether it is in the scene, in a collision and with what, where it stands on the road surfaces,
 * its speed, its distance travelled, and the clearance: the distance from its box to the nearest other box.  The reference asks
 * TERMINAL_CONDITIONS["ego_collision"] / ["ego_off_road"] (state/state.py:397-408) of entities[0] alone; here they are asked
 * of THIS entity.  Plain fp64, IEEE division and square root, nothing fused.
 * The observer is slot so of scenario r; `row` is its SG_F_COLL words as the state holds them (State.collisions(); the resets
 * compute the collisions of the reset state).  An observer that is in State.poses:
 *   flags[o]    SG_ST_PRESENT, and the SG_ST_* bits below
 *   info[o][0]  the number of set bits of row
 *   info[o][1]  the lowest set slot of row, -1 when none
 *   info[o][2]  how many of its 4 box corners lie strictly inside the driveable surface (0..4)
 *   info[o][3]  the slot of the nearest other box, -1 when none
 *   feat[o][0]  |vel[:3]|, as EgoMaxSpeed takes it
 *   feat[o][1]  State.distances (SG_F_DIST)
 *   feat[o][2]  the clearance, +inf when there is no other box
 * The corners are the RR, FR, FL, RL points of Entity.get_bounding_box_points.  A point ON a ring is outside, as everywhere in
 * this library; the surface tests are those of sg_road_info and ego_off_road.
 * The clearance: every OTHER slot e of r that is in State.poses (the presence rule of sg_nearest_entities) is a candidate with
 * the squared gap
 *   gap2 = +0.0 when bit e of row is set; otherwise the smallest of 32 squared distances d2 -- each corner P of one box against
 *   each edge a -> b of the other (edges i -> (i + 1) & 3 of the corner ring), both ways round -- by the rule of
 *   sg_lane_observation:
 *     ex = bx - ax, ey = by - ay, L2 = ex*ex + ey*ey;  wx = px - ax, wy = py - ay, t = (wx*ex + wy*ey) / L2
 *     the closest point is a when L2 == 0 or !(t > 0), b (the stored corner) when t >= 1, otherwise (ax + t*ex, ay + t*ey)
 *     dx, dy = P minus that point, d2 = dx*dx + dy*dy
 *   A d2 that is not finite is skipped; an entity with no finite d2 is not a candidate.
 * The nearest box is the smallest (gap2, slot): info[o][3] its slot, feat[o][2] = sqrt(gap2).  Two disjoint convex quads are
 * closest at a corner of one and an edge of the other, so for boxes that do not meet this is the distance between the fp64
 * corner sets up to rounding.
 * An observer that is NOT in State.poses gets flags = SG_ST_OFF_ROAD alone (the reference's rule for an absent entities[0]),
 * info -1, -1, -1, -1 and feat +0.0.
 * flags: [n], required; info: [n][SG_ST_NINFO], may be NULL; feat: [n][SG_ST_NFEAT] doubles, may be NULL.  Every byte of the
 * arrays given is written.  HOST (outputs_device == 0, synchronous, through the observation scratch) or DEVICE (queued on
 * sg_stream(h), not waited for), as in sg_nearest_entities, and a persistent rollout launch that gave up is reported as there.
 * SG_ERR_INVALID: flags NULL.  SG_ERR_STATE before sg_upload.  A refused call writes nothing and leaves the handle working.
 * One wavefront per observer: the scenario's slots go by in blocks of 64, lane = entity; any scenario width.  Not part of the
 * sg_tick graph. */
#define SG_ST_PRESENT        1u   /* the entity is in State.poses */
#define SG_ST_COLLISION      2u   /* its State.collisions() row is not empty */
#define SG_ST_OFF_ROAD       4u   /* TERMINAL_CONDITIONS["ego_off_road"] asked of THIS entity: not in State.poses, or its pose point not
                                     strictly inside the driveable surface; no networks / a scenario without one = empty surface = set */
#define SG_ST_CORNER_OFF     8u   /* present and at least one box corner not strictly inside the driveable surface */
#define SG_ST_HIT_VEHICLE   16u   /* a slot of its collision row has etype 0 */
#define SG_ST_HIT_PEDESTRIAN 32u  /* ... etype 1 */
#define SG_ST_HIT_OTHER     64u   /* ... any other etype */
#define SG_ST_LAYER_SHIFT    8    /* bits 8..15: the OR of the SG_LAYER_* bits of all polygons strictly containing the pose point */
#define SG_ST_NINFO 4
#define SG_ST_NFEAT 3
int sg_entity_status(sg_handle *h, uint32_t *flags, int32_t *info, double *feat, int32_t outputs_device);

/* The same for every observer of sg_set_observers (n = their number; duplicates each get their rows).  For the observer
 * (r, ego of r) the bytes are those of sg_entity_status for scenario r.  With no observers set: SG_OK, nothing is written
 * (flags may be NULL then). */
int sg_entity_status_observers(sg_handle *h, uint32_t *flags, int32_t *info, double *feat, int32_t outputs_device);

/* Routes: where an entity is supposed to go.  Route j belongs to entity (scenario[j], slot[j]) -- a slot of any kind -- and is
 * the polyline pts[pt_off[j] .. pt_off[j+1]) ([n_pts][2] doubles, in driving order, used as given; pt_off: [n + 1]).  The
 * arrays are HOST arrays; the call copies them into buffers the handle owns.  It waits for the work queued on sg_stream(h) (a
 * queued sg_route_observation may still read the previous routes) and builds one device row per segment a -> b, route by route
 * in point order, exactly as sg_set_lanes and sg_set_driver_policy build theirs -- a, e = b - a, L2 = ex*ex + ey*ey (unfused),
 * len = sqrt(L2), cum = the arclength of a within its route as the sequential fp64 sum of the preceding len (0 for the first
 * segment), b -- per route total = cum + len of its last segment (0 without segments), and a map from the entity to its route:
 * observers are looked up by entity, not by their position in a list.  A route of fewer than two points has no segments.
 * n == 0 clears the routes (the arrays may be NULL then).  sg_upload forgets them; sg_reset, sg_reset_scenarios, sg_step*,
 * sg_set_observers, sg_set_drivers and sg_set_driver_policy keep them (the policy's own paths are separate).  A call that is not
 * refused starts the episode accounting of sg_tick_drivers anew (its arclengths were along other routes).
 * SG_ERR_STATE before sg_upload.  SG_ERR_INVALID: n < 0, a NULL array that is needed, a scenario or slot out of range, a
 * (scenario, slot) pair listed twice, pt_off not starting at 0 or not monotone, 2^31 or more segments, a coordinate that is not
 * finite, a route whose total is not finite.  A refused call leaves the previous routes in place. */
#define SG_ROUTE_MAX_AHEAD 16 /* route points ahead per observer */
#define SG_RT_NINFO 2
#define SG_RT_NFEAT 11        /* + 2 * n_ahead */
int sg_set_routes(sg_handle *h, int64_t n, const int32_t *scenario, const int32_t *slot, const int64_t *pt_off, const double *pts);

/* The route and recorded-track observation of the ego of every scenario (n = n_scenarios observers): where the vehicle is
 * along its route of sg_set_routes, where the route goes next, and how far the vehicle is from where its own recording has it
 * at the current time (the "log divergence" of log-replay simulators).  The reference has no such sensor; the recorded pose is
 * its Trajectory.position_at_t.  Plain fp64 with IEEE division and square root, no fused operation.
 * The observer is slot so of scenario r with pose (px, py, h) and (s, c) = sin, cos of h; t is sg_scenario_state.t of r.  An
 * observer that is NOT in State.poses (the presence rule of sg_nearest_entities) gets info -1, -1 and every feature +0.0.  For
 * an observer that is in State.poses:
 *   the recorded track -- with kn the observer's own knots and n_k their number, (xr, yr, ., hr, ., .) is
 *     Trajectory.position_at_t(t) with the default extrapolate=(False, False): the first knot before its time, the last knot
 *     after its time, the linear interpolation between (a single knot: that knot).  X = xr - px, Y = yr - py, (sr, cr) = sin,
 *     cos of hr:
 *     feat[o][0] X*c + Y*s and feat[o][1] Y*c - X*s, where the recording is in the observer's frame; feat[o][2] sqrt(X*X + Y*Y);
 *     feat[o][3] cr*c + sr*s and feat[o][4] sr*c - cr*s, cos and sin of the recorded heading relative to the observer's
 *     info[o][1]  0 when kn[0].t <= t <= kn[n_k - 1].t, -1 when t is before the first knot, 1 when it is after the last;
 *                 2 with n_k == 0, and feat[o][0..4] are +0.0 then
 *   the route -- over the segments of the observer's route, (d2, dx, dy, t_seg) by the point-to-segment rule of
 *     sg_lane_observation (a segment whose d2 is not finite is skipped); the best segment g is the smallest (d2, index within
 *     the route).  With (ux, uy) = (ex/len, ey/len), or (0, 0) when len == 0:
 *     feat[o][5] ux*dy - uy*dx, the lateral offset, left of the route direction positive; feat[o][6] c*ux + s*uy and feat[o][7]
 *     s*ux - c*uy, cos and sin of the observer's heading relative to the route (not saturated: feat[o][6] < 0 says wrong way);
 *     feat[o][8] s0 = cum + t_seg*len, the arclength along the route; feat[o][9] total - s0; feat[o][10] sqrt(d2)
 *     info[o][0]  g's index within the route
 *     Without a route, or with a route that has no (finite) segment: info[o][0] = -1 and feat[o][5 ..] are +0.0
 *   the look-ahead -- for m = 1..n_ahead, target = s0 + (double)m * spacing.  If target > total the point is b of the route's
 *     last segment.  Otherwise with g' the last segment of the route with cum[g'] <= target (cum is non-decreasing and
 *     cum[0] == 0 <= s0: a binary search) and u = (target - cum[g']) / len[g'] (0 when len[g'] == 0) the point is b of g' when
 *     u >= 1, else (ax + u*ex, ay + u*ey).  With X = x - px, Y = y - py: feat[o][11 + 2(m-1)] = X*c + Y*s and
 *     feat[o][12 + 2(m-1)] = Y*c - X*s.  The rule of sg_lane_observation without the successor walk.
 * feat: [n][SG_RT_NFEAT + 2*n_ahead] doubles, required; info: [n][SG_RT_NINFO], may be NULL.  Every byte of the arrays given is
 * written.  HOST (outputs_device == 0, synchronous, through the observation scratch) or DEVICE (queued on sg_stream(h), not
 * waited for), as in sg_nearest_entities, and a persistent rollout launch that gave up is reported as in sg_entity_status.
 * SG_ERR_INVALID: n_ahead outside 0..SG_ROUTE_MAX_AHEAD, spacing NaN, negative or infinite, feat NULL.  SG_ERR_STATE before
 * sg_upload.  Without sg_set_routes the call succeeds: the track part is filled, the route part is -1 / zeros.  One wavefront
 * per observer tests every segment of its route, 64 at a time; any scenario width.  Not part of the sg_tick graph. */
int sg_route_observation(sg_handle *h, int32_t n_ahead, double spacing, double *feat, int32_t *info, int32_t outputs_device);

/* The same for every observer of sg_set_observers (n = their number; duplicates each get their rows).  For the observer
 * (r, ego of r) the bytes are those of sg_route_observation for scenario r.  With no observers set: SG_OK, nothing is written
 * (feat may be NULL then). */
int sg_route_observation_observers(sg_handle *h, int32_t n_ahead, double spacing, double *feat, int32_t *info, int32_t outputs_device);

/* The time to collision (TTC) of the ego of every scenario (n = n_scenarios observers): when its box will first touch another
 * entity's box if everybody keeps going as they are, for how long the two then overlap, and which face meets first -- the
 * surrogate-safety measure of scenario analysis and the dense shaping / early-termination signal of a learning driver.  The
 * reference has no such sensor: its FutureCollisionDetector (sg_future_collision) replays recordings, which is not the future
 * of a driven entity, and answers with one bit.
 * Two oriented boxes translate with constant velocities over [0, horizon].  Headings are FROZEN: the yaw rate is ignored, so
 * for a turning vehicle the answer is that of the tangent motion at this instant.  Two rectangles are disjoint iff one of their
 * four face normals separates them, so the contact interval is the intersection of four slab intervals.  Plain fp64, IEEE
 * division, nothing fused.
 * The observer is slot so of scenario r with pose (xo, yo, ho), (s, c) = sin, cos of ho, velocity (vxo, vyo) -- the x and y
 * components of State.velocities, as sg_nearest_entities reads them -- and box (Wo, Lo, cxo, cyo) = (width, length, center_x,
 * center_y).  The candidates are every OTHER slot e of r that is in State.poses (the presence rule of sg_nearest_entities),
 * with pose (xe, ye, he), (sn, cn) = sin, cos of he, velocity (vxe, vye) and box (We, Le, cxe, cye):
 *   px = xo + (cxo*c - cyo*s),   py = yo + (cxo*s + cyo*c)          (the box centres, as the driver policy forms them)
 *   qx = xe + (cxe*cn - cye*sn), qy = ye + (cxe*sn + cye*cn)
 *   dx = qx - px, dy = qy - py;  wx = vxe - vxo, wy = vye - vyo;  cr = cn*c + sn*s, sr = sn*c - cn*s
 *   axis 0 (observer, along):  o = dx*c  + dy*s,   l = wx*c  + wy*s,   H = 0.5*Lo + 0.5*(fabs(Le*cr) + fabs(We*sr))
 *   axis 1 (observer, across): o = dy*c  - dx*s,   l = wy*c  - wx*s,   H = 0.5*Wo + 0.5*(fabs(Le*sr) + fabs(We*cr))
 *   axis 2 (other, along):     o = dx*cn + dy*sn,  l = wx*cn + wy*sn,  H = 0.5*Le + 0.5*(fabs(Lo*cr) + fabs(Wo*sr))
 *   axis 3 (other, across):    o = dy*cn - dx*sn,  l = wy*cn - wx*sn,  H = 0.5*We + 0.5*(fabs(Lo*sr) + fabs(Wo*cr))
 *   slab (o, l, H): l == 0: (tn, tf) = (-inf, +inf) when fabs(o) <= H, else (+inf, -inf); otherwise t1 = (-H - o)/l,
 *     t2 = (H - o)/l, tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1
 *   the axes in the order 0 to 3, from tmin = +0.0, tmax = +inf, axis = -1:  if (tn > tmin) { tmin = tn; axis = i; } (the first
 *     strictly larger value wins: a tie keeps the lower axis);  if (tf < tmax) tmax = tf;
 *   a pair where any of the twelve o, l, H is NaN is no contact; otherwise e is a contact iff tmin <= tmax && tmin <= horizon
 *     && tmin < +inf (inclusive; horizon may be +inf)
 *   if bit e of the observer's SG_F_COLL row (State.collisions()) is set, e is a contact with tmin = +0.0 and axis = -1 whatever
 *     the slabs say (tmax and the l stay what the rules above gave): the state's own predicate decides the present, as for the
 *     clearance of sg_entity_status
 * tmin is never negative and never -0.0.  The threat is the contact with the smallest (tmin, slot).
 *   feat[o][0]  tmin of the threat; +inf without one
 *   feat[o][1]  tmax > tmin ? tmax : tmin of the threat, when the overlap ends (possibly +inf); +0.0 without one
 *   feat[o][2]  l of axis 0 and
 *   feat[o][3]  l of axis 1 of the threat: its velocity relative to the observer's in the observer's frame; +0.0 without one
 *   info[o][0]  the threat's slot; -1 without one
 *   info[o][1]  the number of contacts within the horizon
 *   info[o][2]  axis of the threat, the face that meets first: 0 the observer's front or rear, 1 its side, 2 and 3 the other
 *               box's faces; -1 for an overlap that already exists, and without a threat
 * An observer that is not in State.poses gets info -1, -1, -1 and feat +0.0.
 * feat: [n][SG_TTC_NFEAT] doubles, required; info: [n][SG_TTC_NINFO], may be NULL.  Every byte of the arrays given is written.
 * HOST (outputs_device == 0, synchronous, through the observation scratch) or DEVICE (queued on sg_stream(h), not waited for),
 * as in sg_nearest_entities, and a persistent rollout launch that gave up is reported as in sg_entity_status.
 * SG_ERR_INVALID: horizon NaN or negative, feat NULL.  SG_ERR_STATE before sg_upload.  A refused call writes nothing and leaves
 * the handle working.  One wavefront per observer: the scenario's slots go by in blocks of 64, lane = entity; any scenario
 * width.  Not part of the sg_tick graph, and not read by sg_tick_drivers. */
#define SG_TTC_NINFO 3
#define SG_TTC_NFEAT 4
int sg_time_to_collision(sg_handle *h, double horizon, double *feat, int32_t *info, int32_t outputs_device);

/* The same for every observer of sg_set_observers (n = their number; duplicates each get their rows).  For the observer
 * (r, ego of r) the bytes are those of sg_time_to_collision for scenario r.  With no observers set: SG_OK, nothing is written
 * (feat may be NULL then). */
int sg_time_to_collision_observers(sg_handle *h, double horizon, double *feat, int32_t *info, int32_t outputs_device);

/* The surface scan: the static-geometry half of the lidar.  A fan of n_rays beams from the pose point of the ego of every
 * scenario (n = n_scenarios observers), each reporting, for every requested road layer, the range at which the beam first
 * changes side of that layer's surface: an observer standing on the layer gets the distance to leaving it, an observer off it
 * the distance to reaching it.  sg_range_scan sees boxes only (a beam across a kerb comes back with max_range) and
 * sg_entity_status answers yes / no at five points; the reference has no such sensor.  Plain fp64, nothing fused.
 * The observer is slot so of scenario r with pose (xo, yo, ho) and (s, c) = sin, cos of ho.  The beams are those of
 * sg_range_scan: beam b in [0, n_rays) has the angle a_b = angle0 + (double)b * dangle, (sb, cb) = sin, cos of a_b, and the
 * world direction ux = cb*c - sb*s, uy = sb*c + cb*s.  The point of a beam at parameter t is
 *   P(t) = (xo + t*ux, yo + t*uy)                                    (one product and one sum per coordinate)
 * in_l(x, y) is 1 when the point is strictly inside the union of the polygons of scenario r's network that carry the layer
 * bit l -- what sg_road_info_points(...).layers and the SG_ST_LAYER_SHIFT bits of sg_entity_status answer: a point on a ring
 * is outside, a NaN or infinite coordinate is in nothing, and on a handle without networks, or in a scenario without one, it
 * is 0 everywhere.  For layer l = layers[j] and beam b:
 *   1. s0 = in_l(xo, yo): the pose point itself, not P(0); it always agrees with the status bits
 *   2. the coarse march: t_k = (double)k * step for k = 1 .. n_steps; k* is the smallest k with in_l(P(t_k)) != s0
 *   3. without a k* the range is (double)n_steps * step and the beam has no hit
 *   4. otherwise lo = (double)(k* - 1) * step, hi = (double)k* * step, and n_refine times: mid = (lo + hi) * 0.5; when
 *      in_l(P(mid)) != s0, hi = mid, else lo = mid
 *   5. the range is hi, the nearest point KNOWN to lie on the other side; the bracket [lo, hi] around the crossing the march
 *      found has the width step * 2^-n_refine (until lo and hi are adjacent doubles, where it stays)
 * The march samples, it does not intersect: a strip of the other side narrower than `step` that lies between two coarse
 * samples is stepped over, so the caller chooses `step` to suit the narrowest thing it must see.  The scan is defined over the
 * point predicate and not over polygon edges because the boundary of a union is not the union of the polygons' boundaries:
 * abutting lanes and roads share or nearly share edges, which are no crossing at all.
 *   feat[o][j][b]   the range
 *   flags[o][j][b]  bit 0: the beam hit; bit 1: s0.  May be NULL
 *   hits[o][j]      the number of beams that hit.  May be NULL
 * An observer that is not in State.poses gets feat +0.0, flags 0 and hits -1.  Every byte of the arrays given is written.
 * feat: [n][n_layers][n_rays] doubles, flags: [n][n_layers][n_rays] bytes, hits: [n][n_layers]; HOST (outputs_device == 0,
 * synchronous, through the observation scratch) or DEVICE (queued on sg_stream(h), not waited for), as in sg_range_scan, and a
 * persistent rollout launch that gave up is reported as there.  SG_ERR_INVALID: n_layers outside 1..8, a layer that is not
 * exactly one SG_LAYER_* bit (0, the entity layer, is refused here; duplicates are allowed), n_rays outside
 * 1..SG_SURF_MAX_RAYS, angle0 or dangle NaN or infinite, step NaN, infinite or not > 0, n_steps outside 1..SG_SURF_MAX_STEPS,
 * n_refine outside 0..64, feat or layers NULL.  SG_ERR_STATE before sg_upload.  A refused call writes nothing and leaves the
 * handle working.  One wavefront per observer, lane = beam for the march (one cell lookup per sample answers every layer),
 * lane = (beam, layer) for the bisections; it reads nothing of the other entities, so any scenario width.  Not part of the
 * sg_tick graph. */
#define SG_SURF_MAX_RAYS 1024
#define SG_SURF_MAX_STEPS 4096
int sg_surface_scan(sg_handle *h, int32_t n_layers, const int32_t *layers, int32_t n_rays, double angle0, double dangle, double step,
                    int32_t n_steps, int32_t n_refine, double *feat, uint8_t *flags, int32_t *hits, int32_t outputs_device);

/* The same for every observer of sg_set_observers (n = their number; duplicates each get their rows).  For the observer
 * (r, ego of r) the bytes are those of sg_surface_scan for scenario r.  With no observers set: SG_OK, nothing is written
 * (feat may be NULL then). */
int sg_surface_scan_observers(sg_handle *h, int32_t n_layers, const int32_t *layers, int32_t n_rays, double angle0, double dangle,
                              double step, int32_t n_steps, int32_t n_refine, double *feat, uint8_t *flags, int32_t *hits,
                              int32_t outputs_device);

/* One tick of the external-action loop (integrations/openaigym.py:171-226) for every scenario, as one captured hipGraph:
 * sg_step(h, 1, actions) + sg_terminal_flags + sg_raster_map_device with the given observation geometry (1..8 layers).
 * actions: [n_scenarios][2] HOST (actions_device = 0) or DEVICE, or NULL for (0, 0).  Asynchronous: the work is queued on
 * sg_stream(h); *d_obs (DEVICE [R][n_layers][nh][nw] bytes) and *d_flags (DEVICE [R] SG_TERM_* bits) are valid after
 * sg_synchronize(h) until the next observation call.  The graph is rebuilt when the batch, the networks, the time step or
 * the geometry change (or sg_set_rss is switched).  Not for batches with SG_KIND_AGENT_EXTERNAL slots.  With sg_set_rss the
 * captured step runs the RSS callback as sg_step does. */
int sg_tick(sg_handle *h, const double *actions, int32_t actions_device, double width, double height, int32_t nw, int32_t nh,
            int32_t n_layers, const int32_t *layers, const uint8_t **d_obs, const uint32_t **d_flags);

/* RSSDistances.__call__ (metrics/rss/callback.py:58-128) on the current state of every scenario: safe lateral /
 * longitudinal distances between the ego (which must be entity 0, as the reference's callback assumes) and every present
 * entity, the record it appends to that entity's history, and the "unsafe" verdicts the RSS metric reads
 * (metrics/rss/rss.py:70-104).  Call once after sg_reset (reset = 1: forget the histories) and once after every step;
 * scenarios at t == 0.0 are skipped as in the reference.  Asynchronous on sg_stream(h). */
int sg_rss_update(sg_handle *h, int32_t reset);
/* enabled != 0: sg_upload / sg_reset / sg_reset_scenarios / sg_rollout / sg_step / sg_tick run the callback themselves --
 * after the reset and after every step, inside the rollout kernel (any number of steps per launch; also with pedestrian
 * agents and with SG_TERM_EGO_OFF_ROAD) -- as ScenarioGym(state_callbacks=[RSSDistances()]) does.  The line tests of the
 * callback are queued on the device and finished by a second kernel after each launch (queues: env SG_RSSQ_MB, default
 * an eighth of the free device memory and at least 4096 MiB per handle, at most SG_RSSQ_STEPS = 1024 steps per launch; longer
 * calls are cut into several launches; a device short of memory gets shorter launches, not an error).  A scenario that has not stepped since its latest
 * update (it is done) is left alone.  The ego has to be entity 0 (else: one sg_rss_update per step, which says so).
 * Combinations no fused kernel variant carries -- scenarios of more than 512 entities; 257..512 entities with pedestrian
 * agents or SG_TERM_EGO_OFF_ROAD -- run the callback as a launch of its own behind every step: same records. */
int sg_set_rss(sg_handle *h, int32_t enabled);
/* flags [R]: bit 0 = RSS_safe_longitudinal, bit 1 = RSS_safe_lateral (no entity's history holds the corresponding
 * "unsafe_*" record); codes [R*E] of the latest update: 0 safe, 1 lateral, 2 longitudinal, 3 both, 4 unsafe_lateral,
 * 5 unsafe_longitudinal, 6 found, -1 not updated; safe [R*E][2]: lateral, longitudinal safe distance (NaN when not
 * updated).  HOST buffers, each may be NULL. */
int sg_rss_read(sg_handle *h, uint8_t *flags, int32_t *codes, double *safe);

/* CollisionMetric(c_tol) (metrics/collision.py:57-62, default 0.4 rad): the angular half-width of a box corner in
 * get_collision_point; applies to the events classified by the following sg_read_metrics calls. */
int sg_set_collision_tolerance(sg_handle *h, double c_tol);

/* ScenarioGym.get_metrics (scenario_gym.py:308-319): out [R]; events [cap] (may be NULL) */
int sg_read_metrics(sg_handle *h, sg_metrics *out, sg_event *events, int32_t cap, int32_t *n_events);

/* CollisionPointMetric (metrics/collision.py:206-253) for the same events, in the order sg_read_metrics lists them:
 * out[k] = (x, y of the centroid of the two boxes' intersection, (hazard heading - ego heading) mod 2 pi); NaN for a hazard
 * that is itself a controlled agent.  Unlike the type, this is computed for hazards of every catalog type.  HOST [cap][3]. */
int sg_read_collision_points(sg_handle *h, double *out, int32_t cap, int32_t *n_events);

/* State.recorded_poses (state.py:272-290): rows [0, n_rows) of the device record:
 * t_out [n_rows][R], pose_out [n_rows][R*E][6] with NaN for absent entities. HOST buffers. */
int sg_read_record(sg_handle *h, int32_t n_rows, double *t_out, double *pose_out);

/* plain device->host copy of `bytes` from a pointer obtained through sg_state_view_get (after
 * synchronising the handle's stream); lets a ctypes caller read state without any GPU array library */
int sg_copy_to_host(sg_handle *h, const void *device_ptr, void *host_ptr, uint64_t bytes);

/* device time of the last sg_rollout / sg_step call in milliseconds (HIP events on the handle's stream around
 * everything the call enqueued).  Calls of fewer than 16 steps are not timed (the event records would cost more than
 * the kernel of a one-step tick): SG_ERR_STATE after such a call. */
int sg_last_kernel_ms(sg_handle *h, float *ms);

/* the rollout-kernel launches of that call (ONE for the persistent table launch, sg_schedule_info; chunk launches otherwise:
 * long rollouts are cut into chunks of steps so that the controller pre-pass of chunk c+1 overlaps the rollout kernel of
 * chunk c): how many, and the time during which at least one of them was running -- the union of their intervals, each
 * measured with its own HIP event pair on the launch's stream */
int sg_last_launch_stats(sg_handle *h, int32_t *n_launches, float *kernel_ms_total);
/* ... and the plain sum of their durations (what a kernel trace adds up; equal to the union when nothing overlaps) */
int sg_last_launch_gross_ms(sg_handle *h, float *kernel_ms_gross);

/* The launch schedule of the table path (no reference counterpart: scenario_gym/scenario_gym.py:256-267 is one Python loop,
 * and as deterministic as one).  Batches with controlled agents and at least SG_TAB_MIN_STEPS steps to do run as ONE
 * persistent launch (csrc/sgym_queue.hpp): the controller pre-pass and the rollout of every chunk of the time axis in one grid,
 * work items (chunk, block) pulled from a device-side counter -- no timing probe, no dependence on how many hardware queues
 * the process got (rounds 3-4 ran "pipelines" on streams of their own and probed how many overlapped; gone).  Crowds with
 * riders, the in-kernel RSS callback, tiles of several wavefronts and SG_QUEUE=0 take chunk launches on two streams.
 * Results never depend on it.  info[8], all about the last sg_rollout / sg_step call: [0] 0 it did not take the table path,
 * 1 chunk launches, 2 the persistent launch; [1] chunks of the time axis, [2] buffers of the table ring (== [1]: no buffer
 * was reused), [3] wavefronts of the launch (0 unless [0] == 2); [4] wavefronts of the controller pre-pass (controlled lanes
 * / 64), [5] 64-slot blocks of the batch, [6] SIMDs of the device, [7] rollout-kernel launches of the call.
 * A persistent launch whose wavefronts wait longer than SG_QUEUE_TIMEOUT_MS (default 20000) for each other gives up instead
 * of hanging: the next synchronising call returns SG_ERR_HIP and says so. */
int sg_schedule_info(sg_handle *h, int32_t *info);

/* No reference counterpart (diagnostics): the entry point the handle launched last for a step loop -- "sg::rollout_kernel_crowd<4>",
 * "sg::rollout_kernel_tabq_planar<64>", ... -- as a kernel trace of the call names it (without the return type and the argument
 * list).  The string lives in the handle and changes with the next sg_step / sg_rollout / sg_tick.  bench.py reports it as
 * roofline.kernel. */
const char *sg_last_kernel(sg_handle *h);

/* ScenarioGym.rollout (scenario_gym.py:256-267) of a batch whose entities are all replay entities / replay agents is a
 * pure function of the clock except for three ordered sums (State.distances, EgoAvgSpeed, the event list); PID / vehicle
 * agents (controller.py:100-258) never look at another entity, so their poses are a function of the step alone once the
 * controller pre-pass has integrated them (one table for the whole call, filled ahead of the slices).  sg_rollout
 * cuts the time axis of such a batch into slices that run side by side when the batch alone cannot fill the GPU (fewer
 * than 1024 wavefronts -- e.g. one GPU's 512-scenario shard of BASELINE config 4 --, >= 512 steps, no pose recording, no RSS
 * callback, no caller-run agents, no ego_off_road condition): final state, controller state, metrics and events are bit-identical
 * to the step-by-step launch; the states of the intermediate steps are not written to memory (a caller that wants them uses
 * sg_step, record_capacity, or mode 0).  mode: 0 = never, 1 = automatic (default; env SG_SLICE), 2 = whenever the batch
 * is eligible, however short the rollout (tests). */
int sg_set_slicing(sg_handle *h, int32_t mode);

/* Launch policy of sg_rollout / sg_step (results do not depend on it; negative / zero values keep the current one).
 *   tab_min_steps  calls with at least this many steps integrate PID / vehicle agents in the controller pre-pass
 *                  (one lane per agent, 64 agents to a wavefront) instead of inside the rollout kernel
 *                  (default 16, env SG_TAB_MIN_STEPS); scenarios with pedestrian agents always take the in-kernel path
 *   chunk_steps    steps per pre-pass chunk (default 1024, env SG_CHUNK_STEPS)
 *   overlap        1: pre-pass of chunk c+1 runs on a second stream beside the rollout kernel of chunk c (default) */
int sg_set_tuning(sg_handle *h, int32_t tab_min_steps, int32_t chunk_steps, int32_t overlap);

/* test hook: the fp32 sin/cos the collision broad phase and filter use (hardware v_sin_f32 / v_cos_f32 on the
 * fp64-reduced heading).  HOST arrays of n values.  The fp64 results the reference would see
 * (Entity.get_bounding_box_points, entity/base.py:113) are only needed for pairs the fp32 filter cannot decide. */
int sg_debug_trig32(sg_handle *h, int64_t n, const double *heading, float *sin_out, float *cos_out);

/* ---- several devices from one process ----
 * Scenarios are independent (scenario_gym.py:24-27, 178): the batch is cut into contiguous shards of scenarios, one handle
 * per device of `devs`, no exchange during the step loop; cfg->n_scenarios is the TOTAL, cfg->device is ignored.
 * sg_group_upload takes the arrays of the whole batch; sg_group_rollout launches every device before it waits for any;
 * sg_group_read_metrics returns rows and events in whole-batch scenario order.  Everything else (state views, stepping,
 * observations, road networks) goes through the shard's own handle, sg_group_handle(g, i), whose scenarios are
 * [n_scenarios * i / n, n_scenarios * (i + 1) / n).  The multi-process form of the same sharding (one process per GPU,
 * metrics gathered over RCCL) is scenario_gym_amd/distributed.py. */
typedef struct sg_group sg_group;
int sg_group_create(const sg_config *cfg, int32_t n_devices, const int32_t *devs, sg_group **out);
int sg_group_destroy(sg_group *g);
int32_t sg_group_size(const sg_group *g);
sg_handle *sg_group_handle(sg_group *g, int32_t i);
int sg_group_upload(sg_group *g, const sg_scenarios *all);
int sg_group_rollout(sg_group *g, int32_t max_steps);
int sg_group_read_metrics(sg_group *g, sg_metrics *out, sg_event *events, int32_t cap, int32_t *n_events);
const char *sg_group_last_error(const sg_group *g);

#ifdef __cplusplus
}
#endif
#endif
