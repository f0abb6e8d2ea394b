// h_observe.hip -- observations: the RL tick as one graph launch, terminal flags, and -- each one observe() (sgym_host.hpp) behind its
// argument checks -- map, look-ahead, nearest-entity, pose-history, lane-frame, range-scan, route, time-to-collision and surface-scan observations and the episode status of the ego
// and of a list of observers; the lists of (scenario, slot) pairs (check_pairs, EntityList::upload); the path tables (PathTable) and
// the routes.
#include "sgym_host.hpp"

using namespace sgh;

// the layer codes of a map observation: 0 (the entities) or one SG_LAYER_* bit each
static int check_layers(sg_handle *h, const char *who, int32_t n_layers, const int32_t *layers)
{
    for (int k = 0; k < n_layers; ++k) {
        const uint32_t L = (uint32_t)layers[k];
        if (layers[k] < 0 || L > 255u || (L & (L - 1))) return fail(h, SG_ERR_INVALID, "%s: layers[%d]=%d is not 0 or one SG_LAYER_* bit", who, k, layers[k]);
    }
    return SG_OK;
}

// The map layers of every scenario's ego into d = [R][n_layers][nh][nw] on the handle's stream: one launch per group of at
// most eight layers (the kernel takes the codes by value), each writing every byte of its planes.  Returns the first HIP error
// and enqueues nothing after it (sg_tick calls this while capturing).
static hipError_t enqueue_map_layers(sg_handle *h, double width, double height, int32_t nw, int32_t nh, int32_t n_layers, const int32_t *layers,
                                     unsigned char *d)
{
    const size_t plane = (size_t)nw * nh;
    hipError_t e = hipSuccess;
    for (int32_t l0 = 0; l0 < n_layers && e == hipSuccess; l0 += 8) {
        sgl::map_raster(h->stream, h->p, h->road, h->has_road, nullptr, nullptr, h->R, width, height, nw, nh, std::min(n_layers - l0, 8), layers + l0,
                        d + (size_t)l0 * plane, (int64_t)(n_layers * plane));
        e = hipGetLastError();
    }
    return e;
}

// what every map observation refuses first (sg_tick and sg_raster_map_observers take at most eight layers on top of it)
static bool bad_map_geometry(double width, double height, int32_t nw, int32_t nh, int32_t n_layers, const int32_t *layers)
{
    return !layers || n_layers < 1 || nw < 1 || nh < 1 || !(width >= 0.0) || !(height >= 0.0);
}

// The map layers of every scenario's ego, [R][n_layers][nh][nw], through the observation scratch: into the host array `out` (waited
// for), or with out == nullptr left in the scratch for *d_out (on the handle's stream, not waited for)
static int raster_map_launch(sg_handle *h, const char *who, double width, double height, int32_t nw, int32_t nh, int32_t n_layers,
                             const int32_t *layers, uint8_t *out, const uint8_t **d_out)
{
    if (bad_map_geometry(width, height, nw, nh, n_layers, layers)) return fail(h, SG_ERR_INVALID, "%s: bad argument", who);
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (const int rc = check_layers(h, who, n_layers, layers)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t bytes = (size_t)h->R * n_layers * nw * nh;
    if (out)
        return deliver(h, who, false, h->obs, {{out, bytes}}, 0, [&](void *const *d) {
            return enqueue_map_layers(h, width, height, nw, nh, n_layers, layers, static_cast<unsigned char *>(d[0]));
        });
    unsigned char *d = nullptr;
    if (const int rc = scratch(h, h->obs, bytes, &d)) return rc;
    HIP_TRY(h, enqueue_map_layers(h, width, height, nw, nh, n_layers, layers, d));
    *d_out = d;
    return SG_OK;
}

extern "C" int sg_raster_map(sg_handle *h, double width, double height, int32_t nw, int32_t nh, int32_t n_layers,
                             const int32_t *layers, uint8_t *out)
{
    if (!h || !out) return h ? fail(h, SG_ERR_INVALID, "sg_raster_map: bad argument") : SG_ERR_INVALID;
    return raster_map_launch(h, "sg_raster_map", width, height, nw, nh, n_layers, layers, out, nullptr);
}

extern "C" int sg_raster_map_device(sg_handle *h, double width, double height, int32_t nw, int32_t nh, int32_t n_layers,
                                    const int32_t *layers, const uint8_t **d_out)
{
    if (!h || !d_out) return h ? fail(h, SG_ERR_INVALID, "sg_raster_map_device: bad argument") : SG_ERR_INVALID;
    return raster_map_launch(h, "sg_raster_map_device", width, height, nw, nh, n_layers, layers, nullptr, d_out);
}

extern "C" int sg_raster_entities(sg_handle *h, double width, double height, int32_t nw, int32_t nh, uint8_t *out)
{
    if (!h || !out) return h ? fail(h, SG_ERR_INVALID, "sg_raster_entities: bad argument") : SG_ERR_INVALID;
    const int32_t entity_layer = 0;
    return raster_map_launch(h, "sg_raster_entities", width, height, nw, nh, 1, &entity_layer, out, nullptr);
}

// One tick of the RL loop (integrations/openaigym.py:171-226) as ONE graph launch: the step with the policy's actions, the
// terminal conditions of the new state, the map observation.  Four short kernels whose launch and synchronisation
// overheads exceed their run time when issued one by one; captured once per (batch, observation geometry) and replayed.
extern "C" int sg_tick(sg_handle *h, const double *actions, int32_t actions_device, double width, double height, int32_t nw,
                       int32_t nh, int32_t n_layers, const int32_t *layers, const uint8_t **d_obs, const uint32_t **d_flags)
{
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_tick: no scenarios uploaded");
    if (bad_map_geometry(width, height, nw, nh, n_layers, layers) || n_layers > 8)
        return fail(h, SG_ERR_INVALID, "sg_tick: bad observation geometry (1..8 layers)");
    if (h->n_ext > 0) return fail(h, SG_ERR_STATE, "sg_tick: batches with caller-run agents are driven through sg_set_external_poses + sg_step");
    bool grew = false;
    int rc = check_layers(h, "sg_tick", n_layers, layers);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // fixed device addresses for everything the graph's kernels read or write
    const size_t n_act = (size_t)h->R * 2;
    if ((rc = ensure_actions(h, n_act, &grew))) return rc;
    if (grew) ++h->generation;
    if ((rc = h->term_flags.ensure(h, (size_t)h->R * sizeof(uint32_t), &grew))) return rc;
    if (grew) ++h->generation;
    double *const d_actions = h->actions.as<double>();
    uint32_t *const d_term_flags = h->term_flags.as<uint32_t>();
    unsigned char *d = nullptr;
    if ((rc = scratch(h, h->obs, (size_t)h->R * n_layers * nw * nh, &d))) return rc;
    // sg_set_rss: the callback runs after the step, inside the captured launch (like sg_step; without records of a reset --
    // the callback was switched on after sg_upload -- through sg_rss_update after the graph)
    if (h->wide && (rc = ensure_wide(h))) return rc;
    bool rss_tick = false; // (allocations stay outside the capture)
    if ((rc = rss_fused_call(h, true, &rss_tick))) return rc;
    const bool same = h->tick_exec && h->tick_gen == h->generation && h->tick_w == width && h->tick_h == height &&
                      h->tick_rss == rss_tick && h->tick_nw == nw && h->tick_nh == nh && h->tick_nl == n_layers &&
                      std::equal(layers, layers + n_layers, h->tick_layers);
    if (!same) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (const int rcq = check_queue(h)) return rcq; // (a persistent launch that gave up: sticky)
        if (h->tick_exec) { HIP_TRY(h, hipGraphExecDestroy(h->tick_exec)); h->tick_exec = nullptr; }
        hipGraph_t graph = nullptr;
        HIP_TRY(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        // the step as sg_step runs it, never on the table path (one step: not timed); launch_plan does not synchronise
        rc = launch_plan(h, plan_call(h, 1, rss_tick, false), 1, 0, 1, d_actions);
        hipError_t e = hipSuccess;
        if (!rc && h->wide) {
            // scenarios of more than 512 entities: the map layers (the entity layer tile by tile), the terminal conditions by
            // the kernel of sg_terminal_flags
            e = enqueue_map_layers(h, width, height, nw, nh, n_layers, layers, d);
            if (e == hipSuccess) {
                sgl::terminal_flags(dim3((unsigned)h->R), h->stream, h->p, h->cfg.timestep, d_term_flags);
                e = hipGetLastError();
            }
        } else if (!rc) { // the whole observation (map layers + terminal flags) in one launch: every scenario fits one tile
            sgl::map_raster(h->stream, h->p, h->road, h->has_road, nullptr, nullptr, h->R, width, height, nw, nh, n_layers, layers, d,
                            (int64_t)n_layers * nw * nh, d_term_flags);
            e = hipGetLastError();
        }
        hipError_t e2 = hipStreamEndCapture(h->stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess || e2 != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            return fail(h, SG_ERR_HIP, "sg_tick: capture failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        }
        e = hipGraphInstantiate(&h->tick_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { h->tick_exec = nullptr; return fail(h, SG_ERR_HIP, "sg_tick: hipGraphInstantiate: %s", hipGetErrorString(e)); }
        h->tick_gen = h->generation;
        h->tick_rss = rss_tick;
        h->tick_w = width; h->tick_h = height; h->tick_nw = nw; h->tick_nh = nh; h->tick_nl = n_layers;
        std::copy(layers, layers + n_layers, h->tick_layers);
    }
    if (actions)
        HIP_TRY(h, hipMemcpyAsync(d_actions, actions, n_act * sizeof(double), actions_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    else
        HIP_TRY(h, hipMemsetAsync(d_actions, 0, n_act * sizeof(double), h->stream));
    HIP_TRY(h, hipGraphLaunch(h->tick_exec, h->stream));
    if (h->rss_enabled && !rss_tick && (rc = sg_rss_update(h, 0))) return rc;
    h->timed = false;
    if (d_obs) *d_obs = d;
    if (d_flags) *d_flags = d_term_flags;
    return SG_OK;
}

extern "C" int sg_terminal_flags(sg_handle *h, uint32_t *out, const uint32_t **d_out)
{
    if (!h || (!out && !d_out)) return h ? fail(h, SG_ERR_INVALID, "sg_terminal_flags: no output given") : SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_terminal_flags: no scenarios uploaded");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (const int rc = h->term_flags.ensure(h, (size_t)h->R * sizeof(uint32_t))) return rc;
    uint32_t *const d_term_flags = h->term_flags.as<uint32_t>();
    sgl::terminal_flags(dim3((unsigned)h->R), h->stream, h->p, h->cfg.timestep, d_term_flags);
    HIP_TRY(h, hipGetLastError());
    if (out) {
        HIP_TRY(h, hipMemcpyAsync(out, d_term_flags, (size_t)h->R * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (const int rcq = check_queue(h)) return rcq; // (a persistent launch that gave up: sticky)
    }
    if (d_out) *d_out = d_term_flags;
    return SG_OK;
}


// ---- lists of (scenario, slot) pairs: the observers here, the drivers in h_drive.hip, the owners of the routes below ----------------
int sgh::check_pairs(sg_handle *h, const char *who, int64_t n, const int32_t *scenario, const int32_t *slot, unsigned rules)
{
    std::vector<uint8_t> listed((rules & PAIR_ONCE) && n > 0 ? (size_t)h->R * h->E : 0, 0);
    for (int64_t k = 0; k < n; ++k) {
        if (scenario[k] < 0 || scenario[k] >= h->R) return fail(h, SG_ERR_INVALID, "%s: scenario[%lld]=%d out of range", who, (long long)k, scenario[k]);
        if (slot[k] < 0 || slot[k] >= h->E) return fail(h, SG_ERR_INVALID, "%s: slot[%lld]=%d out of range", who, (long long)k, slot[k]);
        const size_t i = (size_t)scenario[k] * h->E + slot[k];
        if ((rules & PAIR_HOLDS_ENTITY) && h->slot_empty[i])
            return fail(h, SG_ERR_INVALID, "%s: slot %d of scenario %d holds no entity (SG_KIND_NONE)", who, slot[k], scenario[k]);
        if ((rules & PAIR_EXTERNAL) && !h->slot_external[i])
            return fail(h, SG_ERR_INVALID, "%s: slot %d of scenario %d is not an SG_KIND_AGENT_EXTERNAL slot", who, slot[k], scenario[k]);
        if (rules & PAIR_ONCE) { // (two drivers of one slot would race on one speed cell and one pose row)
            if (listed[i]) return fail(h, SG_ERR_INVALID, "%s: slot %d of scenario %d is listed twice", who, slot[k], scenario[k]);
            listed[i] = 1;
        }
    }
    return SG_OK;
}

int sgh::EntityList::upload(sg_handle *h, int64_t n_new, const int32_t *scenario, const int32_t *slot)
{
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    n = 0;
    if (const int rc = buf.ensure(h, (size_t)n_new * 2 * sizeof(int32_t))) return rc;
    HIP_TRY(h, hipMemcpy(scenarios(), scenario, (size_t)n_new * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(slots(), slot, (size_t)n_new * sizeof(int32_t), hipMemcpyHostToDevice));
    n = n_new;
    return SG_OK;
}

// ---- observations for any entity: a list of observers (sgym_observers.hpp) -----------------------------------------------
extern "C" int sg_set_observers(sg_handle *h, int64_t n, const int32_t *scenario, const int32_t *slot)
{
    const char *who = "sg_set_observers";
    if (!h) return SG_ERR_INVALID;
    h->observers.n = 0; // a refused call leaves the handle without observers
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (n < 0 || (n > 0 && (!scenario || !slot))) return fail(h, SG_ERR_INVALID, "%s: n < 0 or null array", who);
    if (n > 0x7fffffffLL) return fail(h, SG_ERR_INVALID, "%s: more than 2^31 - 1 observers (one workgroup each: the grid limit)", who);
    if (const int rc = check_pairs(h, who, n, scenario, slot, PAIR_HOLDS_ENTITY)) return rc;
    return n == 0 ? SG_OK : h->observers.upload(h, n, scenario, slot);
}

// Every observation below is observe() (sgym_host.hpp) behind its own argument checks: n observers -- the ego of every scenario
// (observers == false) or the list of sg_set_observers --, the bytes of its output arrays per observer, its launch.  Host outputs
// pass through the observation scratch, one array behind the other in the order of the list (the optional ones only when asked for).
extern "C" int sg_raster_map_observers(sg_handle *h, double width, double height, int32_t nw, int32_t nh, int32_t n_layers,
                                       const int32_t *layers, uint8_t *out, int32_t outputs_device)
{
    const char *who = "sg_raster_map_observers";
    if (!h) return SG_ERR_INVALID;
    if (bad_map_geometry(width, height, nw, nh, n_layers, layers) || n_layers > 8) return fail(h, SG_ERR_INVALID, "%s: bad argument", who);
    if (h->uploaded) // (the layer codes are judged behind the handle's state, which observe() refuses)
        if (const int rc = check_layers(h, who, n_layers, layers)) return rc;
    const size_t bytes_each = (size_t)n_layers * nw * nh;
    return observe(h, who, true, outputs_device, 0, "out", {{out, bytes_each}}, [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
        sgl::map_raster(h->stream, h->p, h->road, h->has_road, d_scen, d_slot, n, width, height, nw, nh, n_layers, layers, static_cast<unsigned char *>(d[0]),
                        (int64_t)bytes_each);
        return hipGetLastError();
    });
}

// ---- the look-ahead (look_ahead_kernel, sgym_observers.hpp): one byte each ---------------------------------------------------
static int future_call(sg_handle *h, const char *who, bool observers, double horizon, int32_t n_samples, uint8_t *out, int32_t outputs_device)
{
    if (n_samples < 1 || !(horizon >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: bad argument", who);
    return observe(h, who, observers, outputs_device, 0, "out", {{out, 1}}, [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
        sgl::look_ahead(h->stream, h->p, d_scen, d_slot, n, horizon, n_samples, static_cast<unsigned char *>(d[0]));
        return hipGetLastError();
    });
}

extern "C" int sg_future_collision(sg_handle *h, double horizon, int32_t n_samples, uint8_t *out)
{
    if (!h || !out) return h ? fail(h, SG_ERR_INVALID, "sg_future_collision: bad argument") : SG_ERR_INVALID;
    return future_call(h, "sg_future_collision", false, horizon, n_samples, out, 0);
}

extern "C" int sg_future_collision_observers(sg_handle *h, double horizon, int32_t n_samples, uint8_t *out, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return future_call(h, "sg_future_collision_observers", true, horizon, n_samples, out, outputs_device);
}

// ---- the nearest-entity vector observation (nearest_kernel, sgym_observers.hpp): [k][8] doubles, [k] slots, a count --------------
static int nearest_call(sg_handle *h, const char *who, bool observers, int32_t k, double radius, double *feat, int32_t *slots,
                        int32_t *count, int32_t outputs_device)
{
    if (k < 1 || k > SG_NEAR_MAX_K) return fail(h, SG_ERR_INVALID, "%s: k=%d outside 1..%d", who, k, SG_NEAR_MAX_K);
    if (!(radius >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: radius is negative or NaN", who);
    return observe(h, who, observers, outputs_device, 0, "feat", {{feat, (size_t)k * 8 * sizeof(double)}, {slots, (size_t)k * sizeof(int32_t)}, {count, sizeof(int32_t)}},
                   [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
                       sgl::nearest(h->stream, h->p, d_scen, d_slot, n, k, radius, static_cast<double *>(d[0]), static_cast<int32_t *>(d[1]),
                                    static_cast<int32_t *>(d[2]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_nearest_entities(sg_handle *h, int32_t k, double radius, double *feat, int32_t *slots, int32_t *count, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return nearest_call(h, "sg_nearest_entities", false, k, radius, feat, slots, count, outputs_device);
}

extern "C" int sg_nearest_entities_observers(sg_handle *h, int32_t k, double radius, double *feat, int32_t *slots, int32_t *count,
                                             int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return nearest_call(h, "sg_nearest_entities_observers", true, k, radius, feat, slots, count, outputs_device);
}

// ---- the pose history (pose_history_kernel, sgym_observers.hpp): [1 + k][n_samples][6] doubles, [k] slots, a count ------------------
static int history_call(sg_handle *h, const char *who, bool observers, int32_t n_samples, int32_t stride, int32_t k, double radius, double *feat,
                        int32_t *slots, int32_t *count, int32_t outputs_device)
{
    if (n_samples < 1 || n_samples > SG_HIST_MAX_SAMPLES) return fail(h, SG_ERR_INVALID, "%s: n_samples=%d outside 1..%d", who, n_samples, SG_HIST_MAX_SAMPLES);
    if (stride < 1 || stride > SG_HIST_MAX_STRIDE) return fail(h, SG_ERR_INVALID, "%s: stride=%d outside 1..%d", who, stride, SG_HIST_MAX_STRIDE);
    if (k < 0 || k > SG_NEAR_MAX_K) return fail(h, SG_ERR_INVALID, "%s: k=%d outside 0..%d", who, k, SG_NEAR_MAX_K);
    if (!(radius >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: radius is negative or NaN", who);
    if (h->cfg.record_capacity <= 0) return fail(h, SG_ERR_STATE, "%s: needs a pose record: the handle was created with record_capacity == 0", who);
    return observe(h, who, observers, outputs_device, 0, "feat",
                   {{feat, (size_t)(1 + k) * n_samples * 6 * sizeof(double)}, {slots, (size_t)k * sizeof(int32_t)}, {count, sizeof(int32_t)}},
                   [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
                       sgl::pose_history(h->stream, h->p, d_scen, d_slot, n, n_samples, stride, k, radius, static_cast<double *>(d[0]),
                                         static_cast<int32_t *>(d[1]), static_cast<int32_t *>(d[2]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_pose_history(sg_handle *h, int32_t n_samples, int32_t stride, int32_t k, double radius, double *feat, int32_t *slots,
                               int32_t *count, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return history_call(h, "sg_pose_history", false, n_samples, stride, k, radius, feat, slots, count, outputs_device);
}

extern "C" int sg_pose_history_observers(sg_handle *h, int32_t n_samples, int32_t stride, int32_t k, double radius, double *feat,
                                         int32_t *slots, int32_t *count, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return history_call(h, "sg_pose_history_observers", true, n_samples, stride, k, radius, feat, slots, count, outputs_device);
}

// ---- the lane-frame vector observation (lane_observation_kernel, sgym_observers.hpp): [k][6 + 2 * n_ahead] doubles, [k] lane
// indices, a count ------------------------------------------------------------------------------------------------------------
static int lane_call(sg_handle *h, const char *who, bool observers, int32_t k, int32_t n_ahead, double spacing, double radius, double *feat,
                     int32_t *lanes, int32_t *count, int32_t outputs_device)
{
    if (k < 1 || k > SG_LANE_MAX_K) return fail(h, SG_ERR_INVALID, "%s: k=%d outside 1..%d", who, k, SG_LANE_MAX_K);
    if (n_ahead < 0 || n_ahead > SG_LANE_MAX_AHEAD) return fail(h, SG_ERR_INVALID, "%s: n_ahead=%d outside 0..%d", who, n_ahead, SG_LANE_MAX_AHEAD);
    if (!(spacing >= 0.0) || std::isinf(spacing)) return fail(h, SG_ERR_INVALID, "%s: spacing is negative, infinite or NaN", who);
    if (!(radius >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: radius is negative or NaN", who);
    return observe(h, who, observers, outputs_device, 0, "feat",
                   {{feat, (size_t)k * (6 + 2 * (size_t)n_ahead) * sizeof(double)}, {lanes, (size_t)k * sizeof(int32_t)}, {count, sizeof(int32_t)}},
                   [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
                       sgl::lane_observation(h->stream, h->p, h->lanes, d_scen, d_slot, n, k, n_ahead, spacing, radius, static_cast<double *>(d[0]),
                                             static_cast<int32_t *>(d[1]), static_cast<int32_t *>(d[2]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_lane_observation(sg_handle *h, int32_t k, int32_t n_ahead, double spacing, double radius, double *feat, int32_t *lanes,
                                   int32_t *count, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return lane_call(h, "sg_lane_observation", false, k, n_ahead, spacing, radius, feat, lanes, count, outputs_device);
}

extern "C" int sg_lane_observation_observers(sg_handle *h, int32_t k, int32_t n_ahead, double spacing, double radius, double *feat,
                                             int32_t *lanes, int32_t *count, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return lane_call(h, "sg_lane_observation_observers", true, k, n_ahead, spacing, radius, feat, lanes, count, outputs_device);
}

// ---- the range scan (range_scan_kernel, sgym_observers.hpp): [n_rays][2] doubles, [n_rays] slots, a hit count ---------------------
static int scan_call(sg_handle *h, const char *who, bool observers, int32_t n_rays, double angle0, double dangle, double max_range, double *feat,
                     int32_t *slots, int32_t *hits, int32_t outputs_device)
{
    if (n_rays < 1 || n_rays > SG_SCAN_MAX_RAYS) return fail(h, SG_ERR_INVALID, "%s: n_rays=%d outside 1..%d", who, n_rays, SG_SCAN_MAX_RAYS);
    if (!std::isfinite(angle0) || !std::isfinite(dangle)) return fail(h, SG_ERR_INVALID, "%s: angle0 or dangle is infinite or NaN", who);
    if (!(max_range >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: max_range is negative or NaN", who);
    return observe(h, who, observers, outputs_device, 0, "feat", {{feat, (size_t)n_rays * 2 * sizeof(double)}, {slots, (size_t)n_rays * sizeof(int32_t)}, {hits, sizeof(int32_t)}},
                   [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
                       sgl::range_scan(h->stream, h->p, d_scen, d_slot, n, n_rays, angle0, dangle, max_range, static_cast<double *>(d[0]),
                                       static_cast<int32_t *>(d[1]), static_cast<int32_t *>(d[2]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_range_scan(sg_handle *h, int32_t n_rays, double angle0, double dangle, double max_range, double *feat, int32_t *slots,
                             int32_t *hits, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return scan_call(h, "sg_range_scan", false, n_rays, angle0, dangle, max_range, feat, slots, hits, outputs_device);
}

extern "C" int sg_range_scan_observers(sg_handle *h, int32_t n_rays, double angle0, double dangle, double max_range, double *feat,
                                       int32_t *slots, int32_t *hits, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return scan_call(h, "sg_range_scan_observers", true, n_rays, angle0, dangle, max_range, feat, slots, hits, outputs_device);
}

// ---- the entity status (entity_status_kernel, sgym_observers.hpp): the doubles first -- [SG_ST_NFEAT] doubles, [SG_ST_NINFO] ints,
// a flag word ---------------------------------------------------------------------------------------------------------------------
static int status_call(sg_handle *h, const char *who, bool observers, uint32_t *flags, int32_t *info, double *feat, int32_t outputs_device)
{
    return observe(h, who, observers, outputs_device, 2, "flags", {{feat, SG_ST_NFEAT * sizeof(double)}, {info, SG_ST_NINFO * sizeof(int32_t)}, {flags, sizeof(uint32_t)}},
                   [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
                       sgl::entity_status(h->stream, h->p, d_scen, d_slot, n, static_cast<uint32_t *>(d[2]), static_cast<int32_t *>(d[1]),
                                          static_cast<double *>(d[0]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_entity_status(sg_handle *h, uint32_t *flags, int32_t *info, double *feat, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return status_call(h, "sg_entity_status", false, flags, info, feat, outputs_device);
}

extern "C" int sg_entity_status_observers(sg_handle *h, uint32_t *flags, int32_t *info, double *feat, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return status_call(h, "sg_entity_status_observers", true, flags, info, feat, outputs_device);
}

// ---- the time to collision (time_to_collision_kernel, sgym_observers.hpp): [SG_TTC_NFEAT] doubles, [SG_TTC_NINFO] ints ------------------
static int ttc_call(sg_handle *h, const char *who, bool observers, double horizon, double *feat, int32_t *info, int32_t outputs_device)
{
    if (!(horizon >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: horizon is negative or NaN", who);
    return observe(h, who, observers, outputs_device, 0, "feat", {{feat, SG_TTC_NFEAT * sizeof(double)}, {info, SG_TTC_NINFO * sizeof(int32_t)}},
                   [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
                       sgl::time_to_collision(h->stream, h->p, d_scen, d_slot, n, horizon, static_cast<double *>(d[0]), static_cast<int32_t *>(d[1]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_time_to_collision(sg_handle *h, double horizon, double *feat, int32_t *info, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return ttc_call(h, "sg_time_to_collision", false, horizon, feat, info, outputs_device);
}

extern "C" int sg_time_to_collision_observers(sg_handle *h, double horizon, double *feat, int32_t *info, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return ttc_call(h, "sg_time_to_collision_observers", true, horizon, feat, info, outputs_device);
}

// ---- the surface scan (surface_scan_kernel, sgym_observers.hpp): the doubles first -- [n_layers][n_rays] doubles, [n_layers] hit
// counts, [n_layers][n_rays] flag bytes ------------------------------------------------------------------------------------------
static int surface_call(sg_handle *h, const char *who, bool observers, int32_t n_layers, const int32_t *layers, int32_t n_rays, double angle0,
                        double dangle, double step, int32_t n_steps, int32_t n_refine, double *feat, uint8_t *flags, int32_t *hits,
                        int32_t outputs_device)
{
    if (n_layers < 1 || n_layers > 8) return fail(h, SG_ERR_INVALID, "%s: n_layers=%d outside 1..8", who, n_layers);
    if (!layers) return fail(h, SG_ERR_INVALID, "%s: null layers", who);
    for (int k = 0; k < n_layers; ++k) {
        const uint32_t L = (uint32_t)layers[k];
        if (layers[k] < 1 || L > 255u || (L & (L - 1))) return fail(h, SG_ERR_INVALID, "%s: layers[%d]=%d is not one SG_LAYER_* bit", who, k, layers[k]);
    }
    if (n_rays < 1 || n_rays > SG_SURF_MAX_RAYS) return fail(h, SG_ERR_INVALID, "%s: n_rays=%d outside 1..%d", who, n_rays, SG_SURF_MAX_RAYS);
    if (!std::isfinite(angle0) || !std::isfinite(dangle)) return fail(h, SG_ERR_INVALID, "%s: angle0 or dangle is infinite or NaN", who);
    if (!std::isfinite(step) || !(step > 0.0)) return fail(h, SG_ERR_INVALID, "%s: step is not positive, infinite or NaN", who);
    if (n_steps < 1 || n_steps > SG_SURF_MAX_STEPS) return fail(h, SG_ERR_INVALID, "%s: n_steps=%d outside 1..%d", who, n_steps, SG_SURF_MAX_STEPS);
    if (n_refine < 0 || n_refine > 64) return fail(h, SG_ERR_INVALID, "%s: n_refine=%d outside 0..64", who, n_refine);
    const size_t cells = (size_t)n_layers * n_rays;
    return observe(h, who, observers, outputs_device, 0, "feat", {{feat, cells * sizeof(double)}, {hits, (size_t)n_layers * sizeof(int32_t)}, {flags, cells}},
                   [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
                       sgl::surface_scan(h->stream, h->p, d_scen, d_slot, n, n_layers, layers, n_rays, angle0, dangle, step, n_steps, n_refine,
                                         static_cast<double *>(d[0]), static_cast<unsigned char *>(d[2]), static_cast<int32_t *>(d[1]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_surface_scan(sg_handle *h, int32_t n_layers, const int32_t *layers, int32_t n_rays, double angle0, double dangle, double step,
                               int32_t n_steps, int32_t n_refine, double *feat, uint8_t *flags, int32_t *hits, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return surface_call(h, "sg_surface_scan", false, n_layers, layers, n_rays, angle0, dangle, step, n_steps, n_refine, feat, flags, hits, outputs_device);
}

extern "C" int sg_surface_scan_observers(sg_handle *h, int32_t n_layers, const int32_t *layers, int32_t n_rays, double angle0, double dangle,
                                         double step, int32_t n_steps, int32_t n_refine, double *feat, uint8_t *flags, int32_t *hits,
                                         int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return surface_call(h, "sg_surface_scan_observers", true, n_layers, layers, n_rays, angle0, dangle, step, n_steps, n_refine, feat, flags, hits,
                        outputs_device);
}

// ---- path tables: the polylines of sg_set_routes below and of sg_set_driver_policy (h_drive.hip) -------------------------------------
void sgh::PathTable::build(int64_t m, const int64_t *pt_off, const double *pts)
{
    const size_t d0 = dbl.size(), i0 = ints.size();
    dbl.resize(d0 + (size_t)m);
    ints.resize(i0 + (size_t)m + 1);
    for (int64_t j = 0; j < m; ++j) { // the rows of sg_set_lanes (h_road.hip), path by path
        const int32_t first = (int32_t)segs.size();
        ints[i0 + (size_t)j] = first;
        dbl[d0 + (size_t)j] = append_segments(segs, pts, pt_off[j], pt_off[j + 1], (int32_t)j, first);
    }
    ints[i0 + (size_t)m] = (int32_t)segs.size();
}

int sgh::PathTable::upload(sg_handle *h, GrowBuf &buf, const double **d_dbl, const sg::LaneSeg **d_seg, const int32_t **d_ints) const
{
    const size_t b_dbl = dbl.size() * sizeof(double), b_seg = segs.size() * sizeof(sg::LaneSeg), b_int = ints.size() * sizeof(int32_t);
    if (const int rc = buf.ensure(h, b_dbl + b_seg + b_int)) return rc;
    unsigned char *base = buf.as<unsigned char>();
    HIP_TRY(h, hipMemcpy(base, dbl.data(), b_dbl, hipMemcpyHostToDevice));
    if (b_seg) HIP_TRY(h, hipMemcpy(base + b_dbl, segs.data(), b_seg, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(base + b_dbl + b_seg, ints.data(), b_int, hipMemcpyHostToDevice));
    *d_dbl = reinterpret_cast<const double *>(base);
    *d_seg = reinterpret_cast<const sg::LaneSeg *>(base + b_dbl);
    *d_ints = reinterpret_cast<const int32_t *>(base + b_dbl + b_seg);
    return SG_OK;
}

// ---- routes and the route / recorded-track observation (route_observation_kernel, sgym_observers.hpp) ------------------------
extern "C" int sg_set_routes(sg_handle *h, int64_t n, const int32_t *scenario, const int32_t *slot, const int64_t *pt_off, const double *pts)
{
    const char *who = "sg_set_routes";
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    // (a refused call leaves the routes as they were: everything is checked before anything is changed)
    if (n < 0 || (n > 0 && (!scenario || !slot || !pt_off))) return fail(h, SG_ERR_INVALID, "%s: n < 0 or null array", who);
    if (n == 0) {
        forget_routes(h);
        forget_episodes(h);
        return SG_OK;
    }
    if (n > (int64_t)h->R * h->E) return fail(h, SG_ERR_INVALID, "%s: more routes than entity slots: a pair is listed twice", who);
    if (const int rc = check_pairs(h, who, n, scenario, slot, PAIR_ONCE)) return rc;
    PathTable t; // doubles: total [n]; ints: route_of [R * EP], then seg_off [n + 1]
    t.ints.assign((size_t)h->R * h->EP, -1);
    int64_t n_seg = 0;
    for (int64_t j = 0; j < n; ++j) {
        t.ints[(size_t)scenario[j] * h->EP + slot[j]] = (int32_t)j;
        if (pt_off[0] != 0 || pt_off[j + 1] < pt_off[j]) return fail(h, SG_ERR_INVALID, "%s: pt_off not monotone from 0", who);
        n_seg += std::max<int64_t>(pt_off[j + 1] - pt_off[j] - 1, 0);
        if (n_seg >= 0x80000000LL) return fail(h, SG_ERR_INVALID, "%s: 2^31 or more segments", who);
    }
    const int64_t n_pts = pt_off[n];
    if (n_pts > 0 && !pts) return fail(h, SG_ERR_INVALID, "%s: null pts", who);
    for (int64_t i = 0; i < 2 * n_pts; ++i)
        if (!std::isfinite(pts[i])) return fail(h, SG_ERR_INVALID, "%s: pts[%lld] is not finite", who, (long long)(i / 2));
    t.segs.reserve((size_t)n_seg);
    t.build(n, pt_off, pts);
    for (int64_t j = 0; j < n; ++j)
        if (!std::isfinite(t.dbl[(size_t)j])) return fail(h, SG_ERR_INVALID, "%s: the length of route %lld is not finite", who, (long long)j);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (a queued sg_route_observation may still read the previous routes)
    forget_routes(h); // (from here on the old routes are gone: a failure of the runtime leaves the handle without any)
    forget_episodes(h); // (the arclengths sg_tick_drivers remembers were along the old routes)
    sg::RouteIndex r{};
    if (const int rc = t.upload(h, h->routes, &r.total, &r.seg, &r.route_of)) return rc;
    r.seg_off = r.route_of + (size_t)h->R * h->EP;
    h->route = r;
    return SG_OK;
}

// [SG_RT_NFEAT + 2 * n_ahead] doubles, [SG_RT_NINFO] ints
static int route_call(sg_handle *h, const char *who, bool observers, int32_t n_ahead, double spacing, double *feat, int32_t *info,
                      int32_t outputs_device)
{
    if (n_ahead < 0 || n_ahead > SG_ROUTE_MAX_AHEAD) return fail(h, SG_ERR_INVALID, "%s: n_ahead=%d outside 0..%d", who, n_ahead, SG_ROUTE_MAX_AHEAD);
    if (!(spacing >= 0.0) || std::isinf(spacing)) return fail(h, SG_ERR_INVALID, "%s: spacing is negative, infinite or NaN", who);
    return observe(h, who, observers, outputs_device, 0, "feat", {{feat, (SG_RT_NFEAT + 2 * (size_t)n_ahead) * sizeof(double)}, {info, SG_RT_NINFO * sizeof(int32_t)}},
                   [&](void *const *d, const int32_t *d_scen, const int32_t *d_slot, int64_t n) {
                       sgl::route_observation(h->stream, h->p, h->route, d_scen, d_slot, n, n_ahead, spacing, static_cast<double *>(d[0]),
                                              static_cast<int32_t *>(d[1]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_route_observation(sg_handle *h, int32_t n_ahead, double spacing, double *feat, int32_t *info, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return route_call(h, "sg_route_observation", false, n_ahead, spacing, feat, info, outputs_device);
}

extern "C" int sg_route_observation_observers(sg_handle *h, int32_t n_ahead, double spacing, double *feat, int32_t *info,
                                              int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    return route_call(h, "sg_route_observation_observers", true, n_ahead, spacing, feat, info, outputs_device);
}
