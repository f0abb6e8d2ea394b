// h_drive.hip -- per-entity vehicle actions: the driver list (sg_set_drivers) and the step that runs the drivers' controllers on
// the device ahead of the batch's step (sg_step_drivers; drive_kernel, sgym_drive.hpp); the built-in policy that makes the actions of
// listed drivers on the device (sg_set_driver_policy, sg_driver_policy_actions, sg_step_drivers_policy; driver_policy_kernel,
// sgym_policy.hpp).
#include "sgym_host.hpp"

using namespace sgh;

extern "C" int sg_set_drivers(sg_handle *h, int64_t n, const int32_t *scenario, const int32_t *slot)
{
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_set_drivers: no scenarios uploaded");
    if (n < 0 || (n > 0 && (!scenario || !slot))) return fail(h, SG_ERR_INVALID, "sg_set_drivers: n < 0 or null array");
    // (a refused call leaves the list as it was: everything is checked before anything is changed)
    std::vector<uint8_t> listed(n > 0 ? (size_t)h->R * h->E : 0, 0);
    for (int64_t k = 0; k < n; ++k) {
        if (scenario[k] < 0 || scenario[k] >= h->R) return fail(h, SG_ERR_INVALID, "sg_set_drivers: scenario[%lld]=%d out of range", (long long)k, scenario[k]);
        if (slot[k] < 0 || slot[k] >= h->E) return fail(h, SG_ERR_INVALID, "sg_set_drivers: slot[%lld]=%d out of range", (long long)k, slot[k]);
        const size_t i = (size_t)scenario[k] * h->E + slot[k];
        if (!h->slot_external[i])
            return fail(h, SG_ERR_INVALID, "sg_set_drivers: slot %d of scenario %d is not an SG_KIND_AGENT_EXTERNAL slot", slot[k], scenario[k]);
        if (listed[i]) // (two lanes would race on one speed cell and one pose row)
            return fail(h, SG_ERR_INVALID, "sg_set_drivers: slot %d of scenario %d is listed twice", slot[k], scenario[k]);
        listed[i] = 1;
    }
    forget_episodes(h); // (the accounting of sg_tick_drivers is per position in the list)
    if (n == 0) {
        h->n_drv = 0;
        forget_driver_policy(h);
        return SG_OK;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (nothing queued reads the previous list any more)
    h->n_drv = 0; // (from here on the old list is gone: a failure of the runtime leaves the handle without drivers)
    forget_driver_policy(h); // (its indices are positions in the old list)
    if (const int rc = h->drivers.ensure(h, (size_t)n * 2 * sizeof(int32_t))) return rc;
    HIP_TRY(h, hipMemcpy(driver_scenarios(h), scenario, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(driver_slots(h), slot, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    h->n_drv = n;
    return SG_OK;
}

extern "C" int sg_step_drivers(sg_handle *h, int32_t n_steps, const double *actions, int32_t actions_device)
{
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_step_drivers: no scenarios uploaded");
    if (h->n_drv == 0) return fail(h, SG_ERR_STATE, "sg_step_drivers: no drivers set (sg_set_drivers)");
    if (n_steps < 1) return fail(h, SG_ERR_INVALID, "sg_step_drivers: n_steps < 1");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t per_step = (size_t)h->n_drv * 2;
    const double *d_act = nullptr; // (null: every driver gets (0, 0))
    if (actions && actions_device) {
        d_act = actions;
    } else if (actions) {
        const size_t n = (size_t)n_steps * per_step;
        if (const int rc = h->drv_actions.ensure(h, n * sizeof(double))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->drv_actions.ptr, actions, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        d_act = h->drv_actions.as<double>();
    }
    // the SG_KIND_AGENT_VEHICLE slots of the batch get (0, 0), as under sg_step(h, 1, NULL, 0)
    if (const int rc = ensure_actions(h, (size_t)h->R * 2)) return rc;
    HIP_TRY(h, hipMemsetAsync(h->actions.ptr, 0, (size_t)h->R * 2 * sizeof(double), h->stream));
    for (int k = 0; k < n_steps; ++k) {
        sgl::drive(h->stream, h->p, h->cfg.timestep, driver_scenarios(h), driver_slots(h), h->n_drv, d_act ? d_act + (size_t)k * per_step : nullptr,
                   h->d_ext);
        HIP_TRY(h, hipGetLastError());
        if (const int rc = step_forced(h, 1, h->actions.as<double>())) return rc;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return check_queue(h);
}

// ---- the built-in driver policy (driver_policy_kernel, sgym_policy.hpp) ------------------------------------------------------
static bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }

extern "C" int sg_set_driver_policy(sg_handle *h, const sg_driver_policy *pol)
{
    const char *who = "sg_set_driver_policy";
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (h->n_drv == 0) return fail(h, SG_ERR_STATE, "%s: no drivers set (sg_set_drivers)", who);
    if (!pol || pol->m == 0) {
        forget_driver_policy(h);
        return SG_OK;
    }
    // (a refused call leaves the policy as it was: everything is checked before anything is changed)
    const int64_t m = pol->m;
    if (m < 0 || !pol->driver || !pol->params || !pol->pt_off) return fail(h, SG_ERR_INVALID, "%s: m < 0 or null array", who);
    for (int64_t j = 0; j < m; ++j) {
        if (pol->driver[j] < 0 || pol->driver[j] >= h->n_drv || (j > 0 && pol->driver[j] <= pol->driver[j - 1]))
            return fail(h, SG_ERR_INVALID, "%s: driver[%lld]=%lld outside the %lld drivers or not strictly ascending", who, (long long)j,
                        (long long)pol->driver[j], (long long)h->n_drv);
        if (pol->pt_off[0] != 0 || pol->pt_off[j + 1] < pol->pt_off[j]) return fail(h, SG_ERR_INVALID, "%s: pt_off not monotone from 0", who);
        const double *q = pol->params + (size_t)j * SG_DP_NPARAM;
        for (int c = 0; c < SG_DP_NPARAM; ++c)
            if (std::isnan(q[c])) return fail(h, SG_ERR_INVALID, "%s: params[%lld][%d] is NaN", who, (long long)j, c);
        if (!positive_finite(q[SG_DP_V0]) || !positive_finite(q[SG_DP_A]) || !positive_finite(q[SG_DP_B]) || !positive_finite(q[SG_DP_K_SOFT]) ||
            !positive_finite(q[SG_DP_GAP_MIN]))
            return fail(h, SG_ERR_INVALID, "%s: V0, A, B, K_SOFT and GAP_MIN of policy driver %lld must be positive and finite", who, (long long)j);
        if (q[SG_DP_T] < 0.0 || q[SG_DP_S0] < 0.0 || q[SG_DP_HALF] < 0.0 || q[SG_DP_REACH] < 0.0 || std::isinf(q[SG_DP_T]) || std::isinf(q[SG_DP_S0]) ||
            std::isinf(q[SG_DP_HALF]))
            return fail(h, SG_ERR_INVALID, "%s: T, S0, HALF (finite) and REACH of policy driver %lld must not be negative", who, (long long)j);
        if (std::isinf(q[SG_DP_K_PSI]) || std::isinf(q[SG_DP_K_E])) return fail(h, SG_ERR_INVALID, "%s: K_PSI or K_E of policy driver %lld is infinite", who, (long long)j);
    }
    const int64_t n_pts = pol->pt_off[m];
    if (n_pts > 0 && !pol->pts) return fail(h, SG_ERR_INVALID, "%s: null pts", who);
    if (n_pts >= 0x7fffffffLL) return fail(h, SG_ERR_INVALID, "%s: 2^31 - 1 or more points", who);
    for (int64_t i = 0; i < 2 * n_pts; ++i)
        if (std::isnan(pol->pts[i])) return fail(h, SG_ERR_INVALID, "%s: pts[%lld] is NaN", who, (long long)(i / 2));
    // the rows of sg_set_lanes (h_road.hip), path by path
    std::vector<sg::LaneSeg> segs;
    std::vector<int32_t> ints((size_t)(2 * m + 1)); // driver [m], then seg_off [m + 1]
    std::vector<double> dbl((size_t)m * (SG_DP_NPARAM + 1)); // params [m][SG_DP_NPARAM], then total [m]
    std::copy(pol->params, pol->params + (size_t)m * SG_DP_NPARAM, dbl.begin());
    for (int64_t j = 0; j < m; ++j) {
        ints[(size_t)j] = (int32_t)pol->driver[j];
        const int32_t first = (int32_t)segs.size();
        ints[(size_t)(m + j)] = first;
        dbl[(size_t)m * SG_DP_NPARAM + j] = append_segments(segs, pol->pts, pol->pt_off[j], pol->pt_off[j + 1], (int32_t)j, first);
    }
    ints[(size_t)(2 * m)] = (int32_t)segs.size();
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (nothing queued reads the previous policy any more)
    forget_driver_policy(h); // (from here on the old policy is gone: a failure of the runtime leaves the handle without one)
    const size_t b_dbl = dbl.size() * sizeof(double), b_seg = segs.size() * sizeof(sg::LaneSeg), b_int = ints.size() * sizeof(int32_t);
    if (const int rc = h->policy.ensure(h, b_dbl + b_seg + b_int)) return rc;
    unsigned char *base = h->policy.as<unsigned char>();
    HIP_TRY(h, hipMemcpy(base, dbl.data(), b_dbl, hipMemcpyHostToDevice));
    if (b_seg) HIP_TRY(h, hipMemcpy(base + b_dbl, segs.data(), b_seg, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(base + b_dbl + b_seg, ints.data(), b_int, hipMemcpyHostToDevice));
    h->pol.params = reinterpret_cast<const double *>(base);
    h->pol.total = h->pol.params + (size_t)m * SG_DP_NPARAM;
    h->pol.seg = reinterpret_cast<const sg::LaneSeg *>(base + b_dbl);
    h->pol.driver = reinterpret_cast<const int32_t *>(base + b_dbl + b_seg);
    h->pol.seg_off = h->pol.driver + m;
    h->n_pol = m;
    return SG_OK;
}

// device scratch of its own: the observation scratch holds what sg_raster_map_device / sg_tick handed out, which stays valid
static int policy_scratch(sg_handle *h, size_t bytes, unsigned char **out)
{
    if (bytes > h->pol_out.cap) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (const int rc = h->pol_out.ensure(h, bytes)) return rc;
    }
    *out = h->pol_out.as<unsigned char>();
    return SG_OK;
}

// Host outputs pass through the scratch, the doubles first: [m][2] actions, then [m][SG_DP_NFEAT] doubles, then [m][SG_DP_NINFO] ints
// (the last two only when asked for).
extern "C" int sg_driver_policy_actions(sg_handle *h, double *actions, int32_t *info, double *feat, int32_t outputs_device)
{
    const char *who = "sg_driver_policy_actions";
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    const int64_t m = h->n_pol;
    if (m == 0) return queue_gave_up(h); // no policy: nothing is written
    if (!actions) return fail(h, SG_ERR_INVALID, "%s: null actions", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return deliver(h, who, outputs_device, policy_scratch,
                   {{actions, (size_t)m * 2 * sizeof(double)}, {feat, (size_t)m * SG_DP_NFEAT * sizeof(double)}, {info, (size_t)m * SG_DP_NINFO * sizeof(int32_t)}}, 0,
                   [&](void *const *d) {
                       sgl::driver_policy(h->stream, h->p, h->pol, driver_scenarios(h), driver_slots(h), m, nullptr, static_cast<double *>(d[0]),
                                          static_cast<int32_t *>(d[2]), static_cast<double *>(d[1]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_step_drivers_policy(sg_handle *h, int32_t n_steps, const double *actions, int32_t actions_device)
{
    const char *who = "sg_step_drivers_policy";
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (h->n_drv == 0) return fail(h, SG_ERR_STATE, "%s: no drivers set (sg_set_drivers)", who);
    if (h->n_pol == 0) return fail(h, SG_ERR_STATE, "%s: no policy set (sg_set_driver_policy)", who);
    if (n_steps < 1) return fail(h, SG_ERR_INVALID, "%s: n_steps < 1", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // the merged actions live in a buffer of the handle: the caller's rows are copied in, the policy's rows written over them step by step
    const size_t per_step = (size_t)h->n_drv * 2, bytes = (size_t)n_steps * per_step * sizeof(double);
    if (const int rc = h->pol_actions.ensure(h, bytes)) return rc;
    double *d_act = h->pol_actions.as<double>();
    if (actions)
        HIP_TRY(h, hipMemcpyAsync(d_act, actions, bytes, actions_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    else
        HIP_TRY(h, hipMemsetAsync(d_act, 0, bytes, h->stream)); // (null: (0, 0) for every driver the policy does not run)
    if (const int rc = ensure_actions(h, (size_t)h->R * 2)) return rc;
    HIP_TRY(h, hipMemsetAsync(h->actions.ptr, 0, (size_t)h->R * 2 * sizeof(double), h->stream));
    for (int k = 0; k < n_steps; ++k) {
        double *act_k = d_act + (size_t)k * per_step;
        sgl::driver_policy(h->stream, h->p, h->pol, driver_scenarios(h), driver_slots(h), h->n_pol, h->pol.driver, act_k, nullptr, nullptr);
        HIP_TRY(h, hipGetLastError());
        sgl::drive(h->stream, h->p, h->cfg.timestep, driver_scenarios(h), driver_slots(h), h->n_drv, act_k, h->d_ext);
        HIP_TRY(h, hipGetLastError());
        if (const int rc = step_forced(h, 1, h->actions.as<double>())) return rc;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return check_queue(h);
}

// ---- one queued step: the body of sg_step_drivers / sg_step_drivers_policy for n_steps = 1 (sg_tick_drivers, h_episode.hip) ---------
int sgh::drivers_step_queued(sg_handle *h, const char *who, const double *actions, int32_t actions_device)
{
    const size_t per_step = (size_t)h->n_drv * 2, bytes = per_step * sizeof(double);
    const auto host_copy = [&](void *dst) { // (the caller's array is free when the call returns)
        HIP_TRY(h, hipMemcpyAsync(dst, actions, bytes, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return (int)SG_OK;
    };
    const double *d_act = nullptr; // (null: every driver gets (0, 0))
    if (h->n_pol > 0) {
        // the merged actions live in a buffer of the handle: the caller's rows are copied in, the policy's rows written over them
        if (const int rc = h->pol_actions.ensure(h, bytes)) return rc;
        double *merged = h->pol_actions.as<double>();
        if (actions && !actions_device) { if (const int rc = host_copy(merged)) return rc; }
        else if (actions) HIP_TRY(h, hipMemcpyAsync(merged, actions, bytes, hipMemcpyDeviceToDevice, h->stream));
        else HIP_TRY(h, hipMemsetAsync(merged, 0, bytes, h->stream));
        d_act = merged;
    } else if (actions && actions_device) {
        d_act = actions;
    } else if (actions) {
        if (const int rc = h->drv_actions.ensure(h, bytes)) return rc;
        if (const int rc = host_copy(h->drv_actions.ptr)) return rc;
        d_act = h->drv_actions.as<double>();
    }
    // the SG_KIND_AGENT_VEHICLE slots of the batch get (0, 0), as under sg_step(h, 1, NULL, 0)
    if (const int rc = ensure_actions(h, (size_t)h->R * 2)) return rc;
    HIP_TRY(h, hipMemsetAsync(h->actions.ptr, 0, (size_t)h->R * 2 * sizeof(double), h->stream));
    if (h->n_pol > 0) {
        sgl::driver_policy(h->stream, h->p, h->pol, driver_scenarios(h), driver_slots(h), h->n_pol, h->pol.driver, h->pol_actions.as<double>(), nullptr,
                           nullptr);
        if (hipGetLastError() != hipSuccess) return fail(h, SG_ERR_HIP, "%s: launching driver_policy_kernel failed", who);
    }
    sgl::drive(h->stream, h->p, h->cfg.timestep, driver_scenarios(h), driver_slots(h), h->n_drv, d_act, h->d_ext);
    if (hipGetLastError() != hipSuccess) return fail(h, SG_ERR_HIP, "%s: launching drive_kernel failed", who);
    return step_forced(h, 1, h->actions.as<double>());
}
