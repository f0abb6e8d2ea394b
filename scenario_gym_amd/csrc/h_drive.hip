// h_drive.hip -- per-entity vehicle actions: the driver list (sg_set_drivers: check_pairs + EntityList::upload) and drivers_step, the
// one step routine that runs the drivers' controllers on the device ahead of the batch's step (drive_kernel, sgym_drive.hpp) with or
// without the built-in policy ahead of them (driver_policy_kernel, sgym_policy.hpp), behind sg_step_drivers, sg_step_drivers_policy
// and sg_tick_drivers; the policy itself (sg_set_driver_policy: a PathTable; sg_driver_policy_actions).
#include "sgym_host.hpp"

using namespace sgh;

extern "C" int sg_set_drivers(sg_handle *h, int64_t n, const int32_t *scenario, const int32_t *slot)
{
    const char *who = "sg_set_drivers";
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (n < 0 || (n > 0 && (!scenario || !slot))) return fail(h, SG_ERR_INVALID, "%s: n < 0 or null array", who);
    // (a refused call leaves the list as it was: everything is checked before anything is changed)
    if (const int rc = check_pairs(h, who, n, scenario, slot, PAIR_EXTERNAL | PAIR_ONCE)) return rc;
    forget_episodes(h); // (the accounting of sg_tick_drivers is per position in the list)
    forget_driver_policy(h); // (its indices are positions in the old list)
    ++h->drivers_gen;        // (... and so are the accounting rows of a snapshot)
    if (n == 0) {
        h->drivers.n = 0;
        return SG_OK;
    }
    return h->drivers.upload(h, n, scenario, slot);
}

// ---- the step of the drivers: what sg_step_drivers, sg_step_drivers_policy and sg_tick_drivers (h_episode.hip) run ----------------
int sgh::drivers_step(sg_handle *h, int n_steps, const double *actions, int32_t actions_device, bool policy, bool wait_host_copy)
{
    const size_t per_step = (size_t)h->drivers.n * 2, bytes = (size_t)n_steps * per_step * sizeof(double);
    const bool host = actions && !actions_device;
    const double *d_act = actions; // (a device buffer is read in place; null: every driver gets (0, 0))
    if (policy || host) {
        // a buffer of the handle: host actions are copied in; under the policy the caller's rows are copied in (null: (0, 0) for every
        // driver the policy does not run) and the policy's rows written over them step by step
        GrowBuf &stage = policy ? h->pol_actions : h->drv_actions;
        if (const int rc = stage.ensure(h, bytes)) return rc;
        if (actions)
            HIP_TRY(h, hipMemcpyAsync(stage.ptr, actions, bytes, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream));
        else
            HIP_TRY(h, hipMemsetAsync(stage.ptr, 0, bytes, h->stream));
        if (host && wait_host_copy) HIP_TRY(h, hipStreamSynchronize(h->stream)); // (the caller's array is free when the call returns)
        d_act = stage.as<double>();
    }
    // the SG_KIND_AGENT_VEHICLE slots of the batch get (0, 0), as under sg_step(h, 1, NULL, 0)
    if (const int rc = ensure_actions(h, (size_t)h->R * 2)) return rc;
    HIP_TRY(h, hipMemsetAsync(h->actions.ptr, 0, (size_t)h->R * 2 * sizeof(double), h->stream));
    for (int k = 0; k < n_steps; ++k) {
        const double *act_k = d_act ? d_act + (size_t)k * per_step : nullptr;
        if (policy) {
            sgl::driver_policy(h->stream, h->p, h->pol, h->drivers.scenarios(), h->drivers.slots(), h->n_pol, h->pol.driver,
                               h->pol_actions.as<double>() + (size_t)k * per_step, nullptr, nullptr);
            HIP_TRY(h, hipGetLastError());
        }
        sgl::drive(h->stream, h->p, h->cfg.timestep, h->drivers.scenarios(), h->drivers.slots(), h->drivers.n, act_k, h->d_ext);
        HIP_TRY(h, hipGetLastError());
        if (const int rc = step_forced(h, 1, h->actions.as<double>())) return rc;
    }
    return SG_OK;
}

extern "C" int sg_step_drivers(sg_handle *h, int32_t n_steps, const double *actions, int32_t actions_device)
{
    const char *who = "sg_step_drivers";
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (h->drivers.n == 0) return fail(h, SG_ERR_STATE, "%s: no drivers set (sg_set_drivers)", who);
    if (n_steps < 1) return fail(h, SG_ERR_INVALID, "%s: n_steps < 1", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (const int rc = drivers_step(h, n_steps, actions, actions_device, false, false)) return rc; // (a policy that is set is not run)
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
    if (h->drivers.n == 0) return fail(h, SG_ERR_STATE, "%s: no drivers set (sg_set_drivers)", who);
    if (!pol || pol->m == 0) {
        forget_driver_policy(h);
        return SG_OK;
    }
    // (a refused call leaves the policy as it was: everything is checked before anything is changed)
    const int64_t m = pol->m;
    if (m < 0 || !pol->driver || !pol->params || !pol->pt_off) return fail(h, SG_ERR_INVALID, "%s: m < 0 or null array", who);
    for (int64_t j = 0; j < m; ++j) {
        if (pol->driver[j] < 0 || pol->driver[j] >= h->drivers.n || (j > 0 && pol->driver[j] <= pol->driver[j - 1]))
            return fail(h, SG_ERR_INVALID, "%s: driver[%lld]=%lld outside the %lld drivers or not strictly ascending", who, (long long)j,
                        (long long)pol->driver[j], (long long)h->drivers.n);
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
        if (q[SG_DP_CORRIDOR] != 0.0 && q[SG_DP_CORRIDOR] != 1.0)
            return fail(h, SG_ERR_INVALID, "%s: CORRIDOR of policy driver %lld is neither 0 (straight) nor 1 (along the path)", who, (long long)j);
    }
    const int64_t n_pts = pol->pt_off[m];
    if (n_pts > 0 && !pol->pts) return fail(h, SG_ERR_INVALID, "%s: null pts", who);
    if (n_pts >= 0x7fffffffLL) return fail(h, SG_ERR_INVALID, "%s: 2^31 - 1 or more points", who);
    for (int64_t i = 0; i < 2 * n_pts; ++i)
        if (std::isnan(pol->pts[i])) return fail(h, SG_ERR_INVALID, "%s: pts[%lld] is NaN", who, (long long)(i / 2));
    PathTable t; // doubles: params [m][SG_DP_NPARAM], then total [m]; ints: driver [m], then seg_off [m + 1]
    t.dbl.assign(pol->params, pol->params + (size_t)m * SG_DP_NPARAM);
    t.ints.assign(pol->driver, pol->driver + m);
    t.build(m, pol->pt_off, pol->pts);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (nothing queued reads the previous policy any more)
    forget_driver_policy(h); // (from here on the old policy is gone: a failure of the runtime leaves the handle without one)
    sg::PolicyIndex q{};
    if (const int rc = t.upload(h, h->policy, &q.params, &q.seg, &q.driver)) return rc;
    q.total = q.params + (size_t)m * SG_DP_NPARAM;
    q.seg_off = q.driver + m;
    for (int64_t j = 0; j < m; ++j) q.n_along += pol->params[(size_t)j * SG_DP_NPARAM + SG_DP_CORRIDOR] != 0.0;
    h->pol = q;
    h->n_pol = m;
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
    return deliver(h, who, outputs_device, h->pol_out,
                   {{actions, (size_t)m * 2 * sizeof(double)}, {feat, (size_t)m * SG_DP_NFEAT * sizeof(double)}, {info, (size_t)m * SG_DP_NINFO * sizeof(int32_t)}}, 0,
                   [&](void *const *d) {
                       sgl::driver_policy(h->stream, h->p, h->pol, h->drivers.scenarios(), h->drivers.slots(), m, nullptr, static_cast<double *>(d[0]),
                                          static_cast<int32_t *>(d[2]), static_cast<double *>(d[1]));
                       return hipGetLastError();
                   });
}

extern "C" int sg_step_drivers_policy(sg_handle *h, int32_t n_steps, const double *actions, int32_t actions_device)
{
    const char *who = "sg_step_drivers_policy";
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (h->drivers.n == 0) return fail(h, SG_ERR_STATE, "%s: no drivers set (sg_set_drivers)", who);
    if (h->n_pol == 0) return fail(h, SG_ERR_STATE, "%s: no policy set (sg_set_driver_policy)", who);
    if (n_steps < 1) return fail(h, SG_ERR_INVALID, "%s: n_steps < 1", who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (const int rc = drivers_step(h, n_steps, actions, actions_device, true, false)) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return check_queue(h);
}
