// h_observe.hip -- observations: the RL tick as one graph launch, terminal flags, map, look-ahead, nearest-entity,
// lane-frame, range-scan and route observations and the episode status of the ego and of a list of observers; the routes.
#include "sgym_host.hpp"

using namespace sgh;

// device scratch shared by the observation entry points: a tick of an RL loop calls them once per step, a hipMalloc /
// hipFree pair per call would cost more than the kernels
static int obs_scratch(sg_handle *h, size_t bytes, unsigned char **out)
{
    if (bytes > h->obs.cap) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (const int rc = h->obs.ensure(h, bytes)) return rc;
        ++h->generation;
    }
    *out = h->obs.as<unsigned char>();
    return SG_OK;
}

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
        return deliver(h, who, false, obs_scratch, {{out, bytes}}, 0, [&](void *const *d) {
            return enqueue_map_layers(h, width, height, nw, nh, n_layers, layers, static_cast<unsigned char *>(d[0]));
        });
    unsigned char *d = nullptr;
    if (const int rc = obs_scratch(h, bytes, &d)) return rc;
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
    if ((rc = obs_scratch(h, (size_t)h->R * n_layers * nw * nh, &d))) return rc;
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

// ---- observations for any entity: a list of observers (sgym_observers.hpp) -----------------------------------------------
// the observer list on the device: the scenarios in the first half of the buffer, the slots in the second
static int32_t *observer_scenarios(const sg_handle *h) { return h->observers.as<int32_t>(); }
static int32_t *observer_slots(const sg_handle *h) { return h->observers.as<int32_t>() + h->observers.cap / (2 * sizeof(int32_t)); }

extern "C" int sg_set_observers(sg_handle *h, int64_t n, const int32_t *scenario, const int32_t *slot)
{
    if (!h) return SG_ERR_INVALID;
    h->n_obs = 0; // a refused call leaves the handle without observers
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_set_observers: no scenarios uploaded");
    if (n < 0 || (n > 0 && (!scenario || !slot))) return fail(h, SG_ERR_INVALID, "sg_set_observers: n < 0 or null array");
    if (n > 0x7fffffffLL) return fail(h, SG_ERR_INVALID, "sg_set_observers: more than 2^31 - 1 observers (one workgroup each: the grid limit)");
    for (int64_t k = 0; k < n; ++k) {
        if (scenario[k] < 0 || scenario[k] >= h->R) return fail(h, SG_ERR_INVALID, "sg_set_observers: scenario[%lld]=%d out of range", (long long)k, scenario[k]);
        if (slot[k] < 0 || slot[k] >= h->E) return fail(h, SG_ERR_INVALID, "sg_set_observers: slot[%lld]=%d out of range", (long long)k, slot[k]);
        if (h->slot_empty[(size_t)scenario[k] * h->E + slot[k]])
            return fail(h, SG_ERR_INVALID, "sg_set_observers: slot %d of scenario %d holds no entity (SG_KIND_NONE)", slot[k], scenario[k]);
    }
    if (n == 0) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (a queued observation call may still read the previous list)
    if (const int rc = h->observers.ensure(h, (size_t)n * 2 * sizeof(int32_t))) return rc;
    HIP_TRY(h, hipMemcpy(observer_scenarios(h), scenario, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(observer_slots(h), slot, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    h->n_obs = n;
    return SG_OK;
}

extern "C" int sg_raster_map_observers(sg_handle *h, double width, double height, int32_t nw, int32_t nh, int32_t n_layers,
                                       const int32_t *layers, uint8_t *out, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    if (bad_map_geometry(width, height, nw, nh, n_layers, layers) || n_layers > 8) return fail(h, SG_ERR_INVALID, "sg_raster_map_observers: bad argument");
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_raster_map_observers: no scenarios uploaded");
    if (const int rc = check_layers(h, "sg_raster_map_observers", n_layers, layers)) return rc;
    if (h->n_obs == 0) return queue_gave_up(h); // no observers: nothing is written
    if (!out) return fail(h, SG_ERR_INVALID, "sg_raster_map_observers: null out");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t bytes_each = (size_t)n_layers * nw * nh;
    return deliver(h, "sg_raster_map_observers", outputs_device, obs_scratch, {{out, (size_t)h->n_obs * bytes_each}}, 0, [&](void *const *d) {
        sgl::map_raster(h->stream, h->p, h->road, h->has_road, observer_scenarios(h), observer_slots(h), h->n_obs, width, height, nw, nh, n_layers,
                        layers, static_cast<unsigned char *>(d[0]), (int64_t)bytes_each);
        return hipGetLastError();
    });
}

// ---- the look-ahead (look_ahead_kernel, sgym_observers.hpp) ---------------------------------------------------------------
// n observers: the ego of every scenario (observers == false) or the list of sg_set_observers; one byte each
static int future_call(sg_handle *h, const char *who, bool observers, double horizon, int32_t n_samples, uint8_t *out, int32_t outputs_device)
{
    if (n_samples < 1 || !(horizon >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: bad argument", who);
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    const int64_t n = observers ? h->n_obs : (int64_t)h->R;
    if (n == 0) return queue_gave_up(h); // no observers: nothing is written
    if (!out) return fail(h, SG_ERR_INVALID, "%s: null out", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int32_t *d_scen = observers ? observer_scenarios(h) : nullptr, *d_slot = observers ? observer_slots(h) : nullptr;
    return deliver(h, who, outputs_device, obs_scratch, {{out, (size_t)n}}, 0, [&](void *const *d) {
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

// ---- the nearest-entity vector observation (nearest_kernel, sgym_observers.hpp) -------------------------------------------
// n observers: the ego of every scenario (observers == false) or the list of sg_set_observers.  Host outputs pass through the
// observation scratch: [n][k][8] doubles, then [n][k] slots, then [n] counts (the last two only when asked for).
static int nearest_call(sg_handle *h, const char *who, bool observers, int32_t k, double radius, double *feat, int32_t *slots,
                        int32_t *count, int32_t outputs_device)
{
    if (k < 1 || k > SG_NEAR_MAX_K) return fail(h, SG_ERR_INVALID, "%s: k=%d outside 1..%d", who, k, SG_NEAR_MAX_K);
    if (!(radius >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: radius is negative or NaN", who);
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    const int64_t n = observers ? h->n_obs : (int64_t)h->R;
    if (n == 0) return queue_gave_up(h); // no observers: nothing is written
    if (!feat) return fail(h, SG_ERR_INVALID, "%s: null feat", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int32_t *d_scen = observers ? observer_scenarios(h) : nullptr, *d_slot = observers ? observer_slots(h) : nullptr;
    const size_t nk = (size_t)n * k;
    return deliver(h, who, outputs_device, obs_scratch, {{feat, nk * 8 * sizeof(double)}, {slots, nk * sizeof(int32_t)}, {count, (size_t)n * sizeof(int32_t)}}, 0,
                   [&](void *const *d) {
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

// ---- the lane-frame vector observation (lane_observation_kernel, sgym_observers.hpp) ---------------------------------------
// n observers as above.  Host outputs pass through the observation scratch: [n][k][6 + 2 * n_ahead] doubles, then [n][k] lane
// indices, then [n] counts (the last two only when asked for).
static int lane_call(sg_handle *h, const char *who, bool observers, int32_t k, int32_t n_ahead, double spacing, double radius, double *feat,
                     int32_t *lanes, int32_t *count, int32_t outputs_device)
{
    if (k < 1 || k > SG_LANE_MAX_K) return fail(h, SG_ERR_INVALID, "%s: k=%d outside 1..%d", who, k, SG_LANE_MAX_K);
    if (n_ahead < 0 || n_ahead > SG_LANE_MAX_AHEAD) return fail(h, SG_ERR_INVALID, "%s: n_ahead=%d outside 0..%d", who, n_ahead, SG_LANE_MAX_AHEAD);
    if (!(spacing >= 0.0) || std::isinf(spacing)) return fail(h, SG_ERR_INVALID, "%s: spacing is negative, infinite or NaN", who);
    if (!(radius >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: radius is negative or NaN", who);
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    const int64_t n = observers ? h->n_obs : (int64_t)h->R;
    if (n == 0) return queue_gave_up(h); // no observers: nothing is written
    if (!feat) return fail(h, SG_ERR_INVALID, "%s: null feat", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int32_t *d_scen = observers ? observer_scenarios(h) : nullptr, *d_slot = observers ? observer_slots(h) : nullptr;
    const size_t nk = (size_t)n * k;
    return deliver(h, who, outputs_device, obs_scratch,
                   {{feat, nk * (6 + 2 * (size_t)n_ahead) * sizeof(double)}, {lanes, nk * sizeof(int32_t)}, {count, (size_t)n * sizeof(int32_t)}}, 0,
                   [&](void *const *d) {
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

// ---- the range scan (range_scan_kernel, sgym_observers.hpp) ----------------------------------------------------------------
// n observers as above.  Host outputs pass through the observation scratch: [n][n_rays][2] doubles, then [n][n_rays] slots, then
// [n] hit counts (the last two only when asked for).
static int scan_call(sg_handle *h, const char *who, bool observers, int32_t n_rays, double angle0, double dangle, double max_range, double *feat,
                     int32_t *slots, int32_t *hits, int32_t outputs_device)
{
    if (n_rays < 1 || n_rays > SG_SCAN_MAX_RAYS) return fail(h, SG_ERR_INVALID, "%s: n_rays=%d outside 1..%d", who, n_rays, SG_SCAN_MAX_RAYS);
    if (!std::isfinite(angle0) || !std::isfinite(dangle)) return fail(h, SG_ERR_INVALID, "%s: angle0 or dangle is infinite or NaN", who);
    if (!(max_range >= 0.0)) return fail(h, SG_ERR_INVALID, "%s: max_range is negative or NaN", who);
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    const int64_t n = observers ? h->n_obs : (int64_t)h->R;
    if (n == 0) return queue_gave_up(h); // no observers: nothing is written
    if (!feat) return fail(h, SG_ERR_INVALID, "%s: null feat", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int32_t *d_scen = observers ? observer_scenarios(h) : nullptr, *d_slot = observers ? observer_slots(h) : nullptr;
    const size_t nb = (size_t)n * n_rays;
    return deliver(h, who, outputs_device, obs_scratch, {{feat, nb * 2 * sizeof(double)}, {slots, nb * sizeof(int32_t)}, {hits, (size_t)n * sizeof(int32_t)}}, 0,
                   [&](void *const *d) {
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

// ---- the entity status (entity_status_kernel, sgym_observers.hpp) ----------------------------------------------------------
// n observers as above.  Host outputs pass through the observation scratch, the doubles first: [n][SG_ST_NFEAT] doubles, then
// [n][SG_ST_NINFO] ints, then [n] flag words (the first two only when asked for).
static int status_call(sg_handle *h, const char *who, bool observers, uint32_t *flags, int32_t *info, double *feat, int32_t outputs_device)
{
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    const int64_t n = observers ? h->n_obs : (int64_t)h->R;
    if (n == 0) return queue_gave_up(h); // no observers: nothing is written
    if (!flags) return fail(h, SG_ERR_INVALID, "%s: null flags", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int32_t *d_scen = observers ? observer_scenarios(h) : nullptr, *d_slot = observers ? observer_slots(h) : nullptr;
    return deliver(h, who, outputs_device, obs_scratch,
                   {{feat, (size_t)n * SG_ST_NFEAT * sizeof(double)}, {info, (size_t)n * SG_ST_NINFO * sizeof(int32_t)}, {flags, (size_t)n * sizeof(uint32_t)}}, 0,
                   [&](void *const *d) {
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
    std::vector<int32_t> ints((size_t)(n + 1) + (size_t)h->R * h->EP, -1); // seg_off [n + 1], then route_of [R * EP]
    int32_t *const route_of = ints.data() + (n + 1);
    int64_t n_seg = 0;
    for (int64_t j = 0; j < n; ++j) {
        if (scenario[j] < 0 || scenario[j] >= h->R) return fail(h, SG_ERR_INVALID, "%s: scenario[%lld]=%d out of range", who, (long long)j, scenario[j]);
        if (slot[j] < 0 || slot[j] >= h->E) return fail(h, SG_ERR_INVALID, "%s: slot[%lld]=%d out of range", who, (long long)j, slot[j]);
        int32_t &of = route_of[(size_t)scenario[j] * h->EP + slot[j]];
        if (of >= 0) return fail(h, SG_ERR_INVALID, "%s: slot %d of scenario %d is listed twice", who, slot[j], scenario[j]);
        of = (int32_t)j;
        if (pt_off[0] != 0 || pt_off[j + 1] < pt_off[j]) return fail(h, SG_ERR_INVALID, "%s: pt_off not monotone from 0", who);
        n_seg += std::max<int64_t>(pt_off[j + 1] - pt_off[j] - 1, 0);
        if (n_seg >= 0x80000000LL) return fail(h, SG_ERR_INVALID, "%s: 2^31 or more segments", who);
    }
    const int64_t n_pts = pt_off[n];
    if (n_pts > 0 && !pts) return fail(h, SG_ERR_INVALID, "%s: null pts", who);
    for (int64_t i = 0; i < 2 * n_pts; ++i)
        if (!std::isfinite(pts[i])) return fail(h, SG_ERR_INVALID, "%s: pts[%lld] is not finite", who, (long long)(i / 2));
    // the rows of sg_set_lanes (h_road.hip), route by route
    std::vector<sg::LaneSeg> segs;
    segs.reserve((size_t)n_seg);
    std::vector<double> total((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        const int32_t first = (int32_t)segs.size();
        ints[(size_t)j] = first;
        total[(size_t)j] = append_segments(segs, pts, pt_off[j], pt_off[j + 1], (int32_t)j, first);
        if (!std::isfinite(total[(size_t)j])) return fail(h, SG_ERR_INVALID, "%s: the length of route %lld is not finite", who, (long long)j);
    }
    ints[(size_t)n] = (int32_t)segs.size();
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (a queued sg_route_observation may still read the previous routes)
    forget_routes(h); // (from here on the old routes are gone: a failure of the runtime leaves the handle without any)
    forget_episodes(h); // (the arclengths sg_tick_drivers remembers were along the old routes)
    const size_t b_dbl = total.size() * sizeof(double), b_seg = segs.size() * sizeof(sg::LaneSeg), b_int = ints.size() * sizeof(int32_t);
    if (const int rc = h->routes.ensure(h, b_dbl + b_seg + b_int)) return rc;
    unsigned char *base = h->routes.as<unsigned char>();
    HIP_TRY(h, hipMemcpy(base, total.data(), b_dbl, hipMemcpyHostToDevice));
    if (b_seg) HIP_TRY(h, hipMemcpy(base + b_dbl, segs.data(), b_seg, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(base + b_dbl + b_seg, ints.data(), b_int, hipMemcpyHostToDevice));
    h->route.total = reinterpret_cast<const double *>(base);
    h->route.seg = reinterpret_cast<const sg::LaneSeg *>(base + b_dbl);
    h->route.seg_off = reinterpret_cast<const int32_t *>(base + b_dbl + b_seg);
    h->route.route_of = h->route.seg_off + (n + 1);
    return SG_OK;
}

// n observers as above.  Host outputs pass through the observation scratch, the doubles first: [n][SG_RT_NFEAT + 2 * n_ahead]
// doubles, then [n][SG_RT_NINFO] ints (only when asked for).
static int route_call(sg_handle *h, const char *who, bool observers, int32_t n_ahead, double spacing, double *feat, int32_t *info,
                      int32_t outputs_device)
{
    if (n_ahead < 0 || n_ahead > SG_ROUTE_MAX_AHEAD) return fail(h, SG_ERR_INVALID, "%s: n_ahead=%d outside 0..%d", who, n_ahead, SG_ROUTE_MAX_AHEAD);
    if (!(spacing >= 0.0) || std::isinf(spacing)) return fail(h, SG_ERR_INVALID, "%s: spacing is negative, infinite or NaN", who);
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    const int64_t n = observers ? h->n_obs : (int64_t)h->R;
    if (n == 0) return queue_gave_up(h); // no observers: nothing is written
    if (!feat) return fail(h, SG_ERR_INVALID, "%s: null feat", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int32_t *d_scen = observers ? observer_scenarios(h) : nullptr, *d_slot = observers ? observer_slots(h) : nullptr;
    return deliver(h, who, outputs_device, obs_scratch,
                   {{feat, (size_t)n * (SG_RT_NFEAT + 2 * (size_t)n_ahead) * sizeof(double)}, {info, (size_t)n * SG_RT_NINFO * sizeof(int32_t)}}, 0,
                   [&](void *const *d) {
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
