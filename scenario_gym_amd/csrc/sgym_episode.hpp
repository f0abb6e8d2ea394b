// sgym_episode.hpp -- episode_kernel: reward, done, progress, episode statistics and the auto-reset mask of one multi-agent tick
// (sg_tick_drivers), and episode_clear_kernel: the accounting of the drivers of freshly reset scenarios starts anew.
//
// What VectorScenarioEnv._step_drivers computes in numpy between its calls, as one element-wise launch behind the kernels that
// produce its inputs (terminal_flags, entity_status and route_observation on the driver list): lane i is scenario i while i < R
// and driver i while i < n_drv, the two halves independent of each other -- a driver lane reads its scenario's flag word itself,
// never what another lane stored.  No LDS, no barrier, no atomic.  Plain fp64, nothing fused (the units are compiled with
// -ffp-contract=off): with the defaults of sg_episode_rules the rewards have the bits numpy gives.
// The definition is that of sg_tick_drivers in include/sgym.h.  Included through sgym_launch.hpp; the kernels are emitted by k_drive.hip
// alone (SG_UNIT_DRIVE), the host units see EpisodeArgs.
#pragma once
#include "sgym_device.hpp"

namespace sg {

// the rules of sg_episode_rules and the arrays of sg_episode_view, as the kernel takes them (all pointers DEVICE)
struct EpisodeArgs {
    uint32_t terminal_mask, bad_env_flags, bad_driver_flags;
    int32_t auto_reset;
    double r_step, r_bad, w_progress;
    int R;
    int64_t n_drv;
    const int32_t *scen;           // [n_drv] the scenario of every driver
    // inputs of this tick
    const uint32_t *term_flags;    // [R]
    const uint32_t *drv_flags;     // [n_drv]
    const double *route_feat;      // [n_drv][SG_RT_NFEAT] (w_progress != 0)
    const int32_t *route_info;     // [n_drv][SG_RT_NINFO] (w_progress != 0)
    // the accounting the handle keeps from tick to tick
    double *prev_s, *acc_return;   // [n_drv]
    uint8_t *prev_ok;              // [n_drv]
    int32_t *acc_length;           // [R]
    // outputs
    uint8_t *env_done, *reset_mask; // [R]
    double *env_reward;             // [R]
    int32_t *ep_length;             // [R]
    double *drv_progress, *drv_reward, *ep_return; // [n_drv]
    uint8_t *drv_done;              // [n_drv]
};

#ifdef SG_UNIT_DRIVE // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void episode_kernel(const EpisodeArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.R) { // the scenario lane
        const uint32_t f = a.term_flags[i];
        const bool done = (f & a.terminal_mask) != 0;
        const bool rs = a.auto_reset != 0 && done;
        a.env_done[i] = done ? 1 : 0;
        a.env_reward[i] = (done && (f & a.bad_env_flags) != 0) ? a.r_bad : a.r_step;
        a.reset_mask[i] = rs ? 1 : 0;
        const int32_t len = a.acc_length[i] + 1;
        a.ep_length[i] = len;
        a.acc_length[i] = rs ? 0 : len;
    }
    if (i < a.n_drv) { // the driver lane
        const int r = a.scen[i];
        const uint32_t f = a.term_flags[r];
        const bool env_done = (f & a.terminal_mask) != 0;
        const bool rs = a.auto_reset != 0 && env_done;
        const bool bad = (a.drv_flags[i] & a.bad_driver_flags) != 0;
        const double base = bad ? a.r_bad : a.r_step;
        double progress = 0.0, reward = base;
        if (a.w_progress != 0.0) {
            const bool on = a.route_info[i * SG_RT_NINFO] >= 0;
            const double s0 = a.route_feat[i * SG_RT_NFEAT + 8];
            if (on && a.prev_ok[i] != 0) progress = s0 - a.prev_s[i];
            const double term = a.w_progress * progress;
            reward = base + term;
            a.prev_s[i] = s0;
            a.prev_ok[i] = (on && !rs) ? 1 : 0;
        }
        a.drv_progress[i] = progress;
        a.drv_reward[i] = reward;
        a.drv_done[i] = (bad || env_done) ? 1 : 0;
        const double ret = a.acc_return[i] + reward;
        a.ep_return[i] = ret;
        a.acc_return[i] = rs ? 0.0 : ret;
    }
}

// sg_reset_scenarios / sg_reset_scenarios_device: the scenarios with mask[r] != 0 and their drivers start their accounting anew
static __global__ __launch_bounds__(256) void episode_clear_kernel(const uint8_t *mask, int R, const int32_t *scen, int64_t n_drv, double *prev_s,
                                                                   double *acc_return, uint8_t *prev_ok, int32_t *acc_length)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < R && mask[i] != 0) acc_length[i] = 0;
    if (i < n_drv && mask[scen[i]] != 0) {
        prev_s[i] = 0.0;
        acc_return[i] = 0.0;
        prev_ok[i] = 0;
    }
}
#endif // SG_UNIT_DRIVE

} // namespace sg
