// sgym_drive.hpp -- drive_kernel: the VehicleController step of the drivers of sg_set_drivers, ahead of a step.
//
// A driver is an SG_KIND_AGENT_EXTERNAL slot whose pose the device produces itself: one lane per driver integrates
// VehicleController._step (controller.py:105-140) from the slot's current pose with the driver's own (accel, steer) and leaves the
// result where every rollout family already looks for the pose of a caller-run agent -- the row of the slot in the handle's
// external-pose buffer (Params::ext_pose).  The step that follows consumes it like a row of sg_set_external_poses; no rollout
// kernel knows about drivers.  The controller's speed lives in the slot's own SG_F_CTRL + 0 cell: the resets write
// `present ? |velocity| : 0` there for every kind, and no rollout family changes the cell of an external lane (the non-table
// families and the wide commit store back what they loaded, the table families never run with external slots).
// Plain fp64, nothing fused; the arithmetic is vehicle_step's (sgym_agents.hpp), called, not restated.
// Included by k_drive.hip alone.
#pragma once
#include "sgym_device.hpp"

namespace sg {

// scen / slot [n]: the drivers; actions [n][2] (accel, steer) in list order or nullptr for (0, 0); ext: [NE][6], the row of
// entity (r, slot) at (r * EP + slot) * 6 as its consumers index it (rollout_body, wide_move_body).
static __global__ __launch_bounds__(256) void drive_kernel(const double *stat, double *dyn, const sg_scenario_state *sdyn, int EP, int FROWS,
                                                           double timestep, const int32_t *scen, const int32_t *slot, int64_t n,
                                                           const double *actions, double *ext)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n) return;
    const int r = scen[d];
    const uint32_t g = (uint32_t)r * (uint32_t)EP + (uint32_t)slot[d];
    const LanePtr st(stat + (size_t)(g >> 6) * (ST_COUNT * 64), (g & 63) * 8u);
    const LanePtr dy(dyn + (size_t)(g >> 6) * ((size_t)FROWS * 64), (g & 63) * 8u);
    double *ep = ext + (size_t)g * 6;
    if (fld<uint64_t>(dy, SG_F_PRESENT) == 0) {
        // not in State.poses (not spawned yet, vanished): "None" -- the step spawns the agent at its trajectory start as it does
        // for every agent (scenario_gym.py:240-244); the speed cell keeps what the reset wrote
        const double nan = __builtin_nan("");
        for (int c = 0; c < 6; ++c) ep[c] = nan;
        return;
    }
    // the clock of the step that follows: the three operations of rollout_body, so dt has the same bits
    const double t = sdyn[r].t, next_t = t + timestep, dt = next_t - t;
    double pose[6];
    for (int c = 0; c < 6; ++c) pose[c] = fld(dy, SG_F_POSE + c);
    CtrlState cs{fld(dy, SG_F_CTRL + 0), 0.0, 0.0, 0.0};
    const double bl = fld(st, ST_BL);
    double aa = 0.0, as = 0.0;
    if (actions) { aa = actions[(size_t)d * 2]; as = actions[(size_t)d * 2 + 1]; }
    ConstTbl K = (ConstTbl)SG_TRIG;
    double sin_h, cos_h; // of the current heading
    sg_sincos(pose[3], sin_h, cos_h, K);
    const LanePtr st_c = st;
    auto cp = [&](int q) -> double { return fld(st_c, ST_CTRL + q); };
    vehicle_step(cs, cp, bl, dt, aa, as, sin_h, cos_h, pose, K); // x, y, h move; z, pitch, roll stay (controller.py:126-131)
    for (int c = 0; c < 6; ++c) ep[c] = pose[c];
    stf(dy, SG_F_CTRL + 0, cs.speed);
}

} // namespace sg
