// k_drive.hip -- drive_kernel: the VehicleController step of the drivers of sg_set_drivers (sgym_drive.hpp); driver_policy_kernel: the
// built-in policy of sg_set_driver_policy, which makes their actions (sgym_policy.hpp); episode_kernel and episode_clear_kernel: the
// rewards, dones and episode statistics of sg_tick_drivers (sgym_episode.hpp).
#define SG_UNIT_DRIVE
#include <algorithm>
#include "sgym_launch.hpp"
#include "sgym_drive.hpp"

namespace sgl {
void drive(hipStream_t s, const sg::Params &p, double timestep, const int32_t *scen, const int32_t *slot, int64_t n, const double *actions,
           double *ext)
{
    if (n <= 0) return;
    sg::drive_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(p.stat, p.dyn, p.sdyn, p.EP, p.FROWS, timestep, scen, slot, n,
                                                                             actions, ext);
}

void driver_policy(hipStream_t s, const sg::Params &p, const sg::PolicyIndex &P, const int32_t *scen, const int32_t *slot, int64_t m,
                   const int32_t *row_of, double *actions, int32_t *info, double *feat)
{
    if (m <= 0) return;
    const dim3 grid((unsigned)((m + 3) / 4));
    if (P.n_along == 0) {
        sg::driver_policy_kernel<false, false><<<grid, dim3(256), 0, s>>>(p, P, scen, slot, m, row_of, actions, info, feat);
    } else if (P.n_along == m) {
        sg::driver_policy_kernel<true, false><<<grid, dim3(256), 0, s>>>(p, P, scen, slot, m, row_of, actions, info, feat);
    } else { // both modes: each instantiation takes the rows of its own
        sg::driver_policy_kernel<false, true><<<grid, dim3(256), 0, s>>>(p, P, scen, slot, m, row_of, actions, info, feat);
        sg::driver_policy_kernel<true, true><<<grid, dim3(256), 0, s>>>(p, P, scen, slot, m, row_of, actions, info, feat);
    }
}

void episode(hipStream_t s, const sg::EpisodeArgs &a)
{
    const int64_t n = std::max<int64_t>(a.R, a.n_drv);
    if (n <= 0) return;
    sg::episode_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(a);
}

void episode_clear(hipStream_t s, const uint8_t *mask, const sg::EpisodeArgs &a)
{
    const int64_t n = std::max<int64_t>(a.R, a.n_drv);
    if (n <= 0) return;
    sg::episode_clear_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(mask, a.R, a.scen, a.n_drv, a.prev_s, a.acc_return, a.prev_ok,
                                                                                     a.acc_length);
}
} // namespace sgl
