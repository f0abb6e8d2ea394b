// k_main.hip -- the setup / read-out / fix-up kernels (sgym_grid.hpp, sgym_sensors.hpp, the fix-ups of sgym_rollout.hpp): one
// launcher per kernel.  Grid and block sizes are the callers'; so is the error handling (hipGetLastError after the call).
#define SG_UNIT_MAIN
#include "sgym_launch.hpp"

// (tests) a launch that does nothing for a while: SG_SLICE_DELAY_US puts one in front of the launch that materialises the last
// step of a time-sliced call, so that anything on the second stream that is NOT ordered behind that launch gets to run first
static __global__ void delay_kernel(long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

namespace sgl {
void event_ego_pose(dim3 grid, hipStream_t s, const sg::Params &p, const sg::TabGroups &tg) { sg::event_ego_pose_kernel<<<grid, dim3(64), 0, s>>>(p, tg); }

void terminal_flags(dim3 grid, hipStream_t s, const sg::Params &p, double timestep, uint32_t *out)
{
    sg::terminal_flags_kernel<<<grid, dim3(64), 0, s>>>(p, timestep, out);
}

void classify_events(dim3 grid, hipStream_t s, const sg::Params &p, double c_tol) { sg::classify_events_kernel<<<grid, dim3(64), 0, s>>>(p, c_tol); }

void rss(dim3 grid, dim3 block, hipStream_t s, const sg::Params &p, int reset, int32_t *rss_state, int32_t *code, double *safe, int32_t *seen)
{
    sg::rss_kernel<<<grid, block, 0, s>>>(p, reset, rss_state, code, safe, seen);
}

void ego_off_road(dim3 grid, hipStream_t s, const sg::Params &p) { sg::ego_off_road_kernel<<<grid, dim3(64), 0, s>>>(p); }

void replay_fixup(int G, dim3 grid, hipStream_t s, const sg::Params &p, const sg::SliceArgs &sa, const int *n_final)
{
#define CALL(G_) sg::replay_fixup_kernel<G_><<<grid, dim3(64), 0, s>>>(p, sa, n_final)
    SGL_DISPATCH_G(G, CALL);
#undef CALL
}

void replay_scenario_fixup(dim3 grid, hipStream_t s, const sg::Params &p, const sg::SliceArgs &sa, const int *n_final, const int *done_in)
{
    sg::replay_scenario_fixup_kernel<<<grid, dim3(64), 0, s>>>(p, sa, n_final, done_in);
}

void slice_final(dim3 grid, hipStream_t s, const sg::Params &p, const sg::SliceArgs &sa, int *n_final, int *done_out)
{
    sg::slice_final_kernel<<<grid, dim3(64), 0, s>>>(p, sa, n_final, done_out);
}

void clock(dim3 grid, hipStream_t s, const double *t0, int n_clocks, double timestep, int n_total, double *tt)
{
    sg::clock_kernel<<<grid, dim3(64), 0, s>>>(t0, n_clocks, timestep, n_total, tt);
}

void delay(hipStream_t s, long long ticks) { delay_kernel<<<dim3(1), dim3(64), 0, s>>>(ticks); }

void build_grid(dim3 grid, hipStream_t s, const sg::Params &p, const int32_t *row_scen, int64_t row0, int64_t row_end)
{
    sg::build_grid_kernel<<<grid, dim3(256), 0, s>>>(p, row_scen, row0, row_end);
}

void trig32(dim3 grid, hipStream_t s, const double *h, float *sin_out, float *cos_out, int64_t n)
{
    sg::trig32_kernel<<<grid, dim3(256), 0, s>>>(h, sin_out, cos_out, n);
}
} // namespace sgl
