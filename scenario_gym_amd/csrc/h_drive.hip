// h_drive.hip -- per-entity vehicle actions: the driver list (sg_set_drivers) and the step that runs the drivers' controllers on
// the device ahead of the batch's step (sg_step_drivers; drive_kernel, sgym_drive.hpp).
#include "sgym_host.hpp"

using namespace sgh;

// the driver list on the device: the scenarios in the first half of the buffer, the slots in the second
static int32_t *driver_scenarios(const sg_handle *h) { return h->drivers.as<int32_t>(); }
static int32_t *driver_slots(const sg_handle *h) { return h->drivers.as<int32_t>() + h->drivers.cap / (2 * sizeof(int32_t)); }

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
    if (n == 0) {
        h->n_drv = 0;
        return SG_OK;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (nothing queued reads the previous list any more)
    h->n_drv = 0; // (from here on the old list is gone: a failure of the runtime leaves the handle without drivers)
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
