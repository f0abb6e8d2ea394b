// sgym_launch.hpp -- host-side launchers of the rollout kernel families.
//
// libsgym_hip.so is linked from one object per kernel family (k_*.hip: `make -j` compiles them side by side, and an
// experiment on one family rebuilds one object); every object includes sgym_device.hpp and instantiates only the entry
// points its launcher names.  The host units (sgym_hip.hip and h_*.hip: the C ABI, sgym_host.hpp) call the launchers below and
// hold no kernel themselves; the setup / read-out / fix-up kernels are k_main.hip's.
// Tile shapes: WV == 1 with G in {4, 8, 16, 32, 64} lanes per scenario, or G == 64 with WV in {2, 4} wavefronts per
// scenario (the plain variant also 8).
#pragma once
#include "sgym_device.hpp"
#include "sgym_wide.hpp"
#include "sgym_queue.hpp"
#include "sgym_policy.hpp"
#include "sgym_episode.hpp"
#include "sgym_snapshot.hpp"

namespace sgl {

// what every rollout_kernel* entry point that runs its controllers in the kernel takes
struct RolloutArgs {
    const sg::Params *p;
    double timestep;
    int n_steps, do_reset, force;
    const double *actions; // [n][R][2] or nullptr
    const double *tab;     // controller table planes or nullptr
};

// k_plain.hip: rollout_kernel<G, WV, false, tab>  (WV == 8: rollout_kernel<64, 8, false, false>)
void rollout_plain(int G, int WV, bool tab, dim3 grid, hipStream_t s, const RolloutArgs &a);
// k_ped.hip: rollout_kernel<max(G, 16), WV, true, false> / rollout_kernel_rss_ped (rss)
void rollout_ped(int G, int WV, bool rss, dim3 grid, hipStream_t s, const RolloutArgs &a);
void rollout_ped_rss(int G, int WV, dim3 grid, hipStream_t s, const RolloutArgs &a); // (k_ped_rss.hip, through rollout_ped)
// k_crowd.hip: rollout_kernel_crowd<WV> / rollout_kernel_crowd_models<WV> / rollout_kernel_crowd_riders<WV>
void rollout_crowd(int WV, bool riders, dim3 grid, hipStream_t s, const RolloutArgs &a, bool models = false);
// k_wide.hip (sgym_wide.hpp): one step (mode 0) or State.reset (mode 1 / 2) of scenarios of more than 512 entities, four kernels
void wide_step(dim3 grid_entities, dim3 grid_scenarios, hipStream_t s, const sg::Params &p, double timestep, const sg::WideArgs &wa,
               bool no_peds /* move + commit as one launch */);
void wide_running(hipStream_t s, const sg::Params &p, int *host_word); // scenarios not done yet -> a word of page-locked host memory
// k_rss.hip: rollout_kernel_rss<G, WV> / rollout_kernel_rss_road<G, WV> (road)
void rollout_rss(int G, int WV, bool road, dim3 grid, hipStream_t s, const RolloutArgs &a);
void rollout_rss_road(int G, int WV, dim3 grid, hipStream_t s, const RolloutArgs &a); // (k_rss_road.hip, through rollout_rss)
// k_rss_tab.hip: rollout_kernel_rss_tab<G> + rss_lines_kernel
void rollout_rss_tab(int G, dim3 grid, hipStream_t s, const sg::Params &p, double timestep, int force, const sg::TabGroups &tg);
void rss_lines(dim3 grid, hipStream_t s, const sg::Params &p, const sg::TabGroups &tg);
// k_road.hip: rollout_kernel_road<G, WV>
void rollout_road(int G, int WV, dim3 grid, hipStream_t s, const RolloutArgs &a);
// k_geom.hip (sgym_geom.hpp): road_info_kernel, one lane per query -- the entity slots of the batch (xy == nullptr, n = R * E) or n
// caller-supplied points; all pointers DEVICE
void road_info(hipStream_t s, const sg::Params &p, const sg::RoadIndex &R, const sg::RoadGeom &G, bool has_road, const int32_t *scen,
               const double *xy, int64_t n, int cap, int32_t *count, int32_t *geoms, uint32_t *layers);
// k_obs.hip (sgym_observers.hpp): map_raster_kernel / look_ahead_kernel, one workgroup per observer k < n: (scen[k], slot[k]), or
// -- scen == nullptr, n = p.R -- the ego of scenario k.  scen / slot / out / flags DEVICE, layers HOST (1..8 codes of
// sg_raster_map).  Layer l of observer k goes to out + k * stride + l * nh * nw; look_ahead: out [n] bytes.
// flags != nullptr (egos only, scenarios of at most 512 entities): the TICK instantiation, which also writes the SG_TERM_* bits.
void map_raster(hipStream_t s, const sg::Params &p, const sg::RoadIndex &R, bool has_road, const int32_t *scen, const int32_t *slot, int64_t n,
                double width, double height, int nw, int nh, int n_layers, const int32_t *layers, unsigned char *out, int64_t stride,
                uint32_t *flags = nullptr);
void look_ahead(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, double horizon, int n_samples,
                unsigned char *out);
// nearest_kernel<NB>: the k <= 32 nearest present entities within `radius` of observer o < n (the same two lists), ascending
// (squared distance, slot).  feat [n][k][8], slots [n][k] (or nullptr), count [n] (or nullptr), all DEVICE.  One wavefront per
// observer for scenarios of at most 512 entities (NB = 1, 2, 4, 8 blocks of 64 slots), one workgroup beyond (NB = 0).
void nearest(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, int k, double radius, double *feat,
             int32_t *slots, int32_t *count);
// pose_history_kernel<NB>: the last n_samples <= SG_HIST_MAX_SAMPLES rows of the pose record (p.rec_cap > 0), `stride` rows apart, of
// observer o < n (the same two lists) and of its k <= 32 neighbours of nearest_kernel, in the observer's current frame.  feat
// [n][1 + k][n_samples][6], slots [n][k] (or nullptr), count [n] (or nullptr), all DEVICE.  The widths of nearest_kernel.
void pose_history(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, int n_samples, int stride, int k,
                  double radius, double *feat, int32_t *slots, int32_t *count);
// lane_observation_kernel: the k <= 8 nearest lane centre lines within `radius` of observer o < n (the same two lists) and
// n_ahead <= 16 points ahead on each.  feat [n][k][6 + 2 * n_ahead], lanes [n][k] (or nullptr), count [n] (or nullptr), all DEVICE;
// L: the rows of sg_set_lanes (L.seg == nullptr: none set).  One wavefront per observer.
void lane_observation(hipStream_t s, const sg::Params &p, const sg::LaneIndex &L, const int32_t *scen, const int32_t *slot, int64_t n, int k,
                      int n_ahead, double spacing, double radius, double *feat, int32_t *lanes, int32_t *count);
// range_scan_kernel: n_rays <= SG_SCAN_MAX_RAYS beams from observer o < n (the same two lists) at angle0 + b * dangle from its
// heading, each against the boxes of the other present entities up to max_range.  feat [n][n_rays][2] (range, range rate), slots
// [n][n_rays] (or nullptr), hits [n] (or nullptr), all DEVICE.  One wavefront per observer, any scenario width.
void range_scan(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, int n_rays, double angle0, double dangle,
                double max_range, double *feat, int32_t *slots, int32_t *hits);
// entity_status_kernel: the episode status of observer o < n (the same two lists): flags [n] SG_ST_* bits, info [n][SG_ST_NINFO] (or
// nullptr), feat [n][SG_ST_NFEAT] (or nullptr), all DEVICE.  One wavefront per observer, any scenario width.
void entity_status(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, uint32_t *flags, int32_t *info,
                   double *feat);
// route_observation_kernel: where observer o < n (the same two lists) is relative to its route of sg_set_routes (P.route_of ==
// nullptr: none set) with n_ahead <= SG_ROUTE_MAX_AHEAD points ahead, and relative to its own recording at the scenario's time.
// feat [n][SG_RT_NFEAT + 2 * n_ahead], info [n][SG_RT_NINFO] (or nullptr), all DEVICE.  One wavefront per observer, any scenario width.
void route_observation(hipStream_t s, const sg::Params &p, const sg::RouteIndex &P, const int32_t *scen, const int32_t *slot, int64_t n,
                       int n_ahead, double spacing, double *feat, int32_t *info);
// time_to_collision_kernel: when the box of observer o < n (the same two lists) first touches another present entity's within `horizon`
// (which may be +inf) if both keep their velocity and heading.  feat [n][SG_TTC_NFEAT], info [n][SG_TTC_NINFO] (or nullptr), all
// DEVICE.  One wavefront per observer, any scenario width.
void time_to_collision(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, double horizon, double *feat,
                       int32_t *info);
// surface_scan_kernel: n_rays <= SG_SURF_MAX_RAYS beams from observer o < n (the same two lists), the beams of range_scan, each against
// the surfaces of the n_layers <= 8 road layers `layers` (HOST, one SG_LAYER_* bit each; they travel by value): n_steps samples `step`
// apart, then n_refine bisections of the step that changed side.  feat [n][n_layers][n_rays], flags [n][n_layers][n_rays] (or
// nullptr), hits [n][n_layers] (or nullptr), all DEVICE.  One wavefront per observer, any scenario width.
void surface_scan(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, int n_layers, const int32_t *layers,
                  int n_rays, double angle0, double dangle, double step, int n_steps, int n_refine, double *feat, unsigned char *flags,
                  int32_t *hits);
// k_drive.hip (sgym_drive.hpp): drive_kernel, one lane per driver d < n: the VehicleController step of entity (scen[d], slot[d]) with
// actions[d] = (accel, steer) (nullptr: (0, 0)) from its current pose, into row (scen[d] * EP + slot[d]) of ext, the handle's
// external-pose buffer [NE][6] -- NaN for a driver that is not in the scene; the controller speed in the slot's SG_F_CTRL + 0 cell.
// All pointers DEVICE.
void drive(hipStream_t s, const sg::Params &p, double timestep, const int32_t *scen, const int32_t *slot, int64_t n, const double *actions,
           double *ext);
// driver_policy_kernel (sgym_policy.hpp): the built-in policy for policy driver o < m, driver P.driver[o] of the list (scen, slot): its
// (accel, steer) on the current state into row (row_of ? row_of[o] : o) of actions [..][2], info [m][SG_DP_NINFO] (or nullptr), feat
// [m][SG_DP_NFEAT] (or nullptr).  One wavefront per policy driver, any scenario width.  All pointers DEVICE.
void driver_policy(hipStream_t s, const sg::Params &p, const sg::PolicyIndex &P, const int32_t *scen, const int32_t *slot, int64_t m,
                   const int32_t *row_of, double *actions, int32_t *info, double *feat);
// episode_kernel (sgym_episode.hpp): reward, done, progress, episode statistics and the reset mask of one sg_tick_drivers, one lane per
// index i < max(a.R, a.n_drv); episode_clear_kernel: the accounting of the scenarios with mask[r] != 0 and of their drivers zeroed.
// All pointers DEVICE.
void episode(hipStream_t s, const sg::EpisodeArgs &a);
void episode_clear(hipStream_t s, const uint8_t *mask, const sg::EpisodeArgs &a);
// k_snap.hip (sgym_snapshot.hpp): snapshot_copy_kernel, one launch -- the rows of the scenarios with mask[r] != 0 (DEVICE [R]; nullptr:
// every scenario) of every segment of the table, handle -> snapshot (restore == 0) or back; a capped grid that strides over the chunks
void snapshot_copy(hipStream_t s, const sg::SnapTable &t, const uint8_t *mask, int restore);
// k_tab.hip: rollout_kernel_tab<G> / rollout_kernel_tab_planar<G>
void rollout_tab(int G, bool planar, dim3 grid, hipStream_t s, const sg::Params &p, double timestep, int force, const sg::TabGroups &tg);
// k_tabq.hip (sgym_queue.hpp): rollout_kernel_tabq<G> / rollout_kernel_tabq_planar<G> -- the table path as one persistent launch
void rollout_tabq(int G, bool planar, dim3 grid, hipStream_t s, const sg::Params &p, double timestep, int force, const sg::TabQueue &tq);
int tabq_waves_per_cu(int G, bool planar); // resident wavefronts of that kernel per compute unit (occupancy query; 0: unknown)
int rss_tabq_waves_per_cu(int G);          // (k_rss_tab.hip)
// k_rss_tab.hip: rollout_kernel_rss_tabq<G> -- the same launch with the RSS callback in the step loop
void rollout_rss_tabq(int G, dim3 grid, hipStream_t s, const sg::Params &p, double timestep, int force, const sg::TabQueue &tq);
// k_slice.hip: rollout_kernel_slice<G> / rollout_kernel_slice_tab<G> (tab != nullptr)
void rollout_slice(int G, dim3 grid, hipStream_t s, const sg::Params &p, double timestep, const sg::SliceArgs &sa, const double *tab);
// k_ctl.hip: the controller pre-pass.  which: 0 control_kernel, 1 control_kernel_riders, 2 control_kernel_fast
enum { CTL_GENERAL = 0, CTL_RIDERS = 1, CTL_FAST = 2 };
void control(int which, dim3 grid, hipStream_t s, const sg::Params &p, double timestep, int n_steps, int first, int k0,
             const double *actions, double *tab, int row0, int metrics);
// k_main.hip: the setup / read-out / fix-up kernels, one launcher per kernel (the block is an argument where the call sites differ)
void event_ego_pose(dim3 grid, hipStream_t s, const sg::Params &p, const sg::TabGroups &tg);
void terminal_flags(dim3 grid, hipStream_t s, const sg::Params &p, double timestep, uint32_t *out);
void classify_events(dim3 grid, hipStream_t s, const sg::Params &p, double c_tol);
void rss(dim3 grid, dim3 block, hipStream_t s, const sg::Params &p, int reset, int32_t *rss_state, int32_t *code, double *safe, int32_t *seen);
void ego_off_road(dim3 grid, hipStream_t s, const sg::Params &p);
void replay_fixup(int G, dim3 grid, hipStream_t s, const sg::Params &p, const sg::SliceArgs &sa, const int *n_final);
void replay_scenario_fixup(dim3 grid, hipStream_t s, const sg::Params &p, const sg::SliceArgs &sa, const int *n_final, const int *done_in);
void slice_final(dim3 grid, hipStream_t s, const sg::Params &p, const sg::SliceArgs &sa, int *n_final, int *done_out);
void clock(dim3 grid, hipStream_t s, const double *t0, int n_clocks, double timestep, int n_total, double *tt);
void delay(hipStream_t s, long long ticks); // (tests) one wavefront that does nothing for `ticks` of the 100 MHz clock
void build_grid(dim3 grid, hipStream_t s, const sg::Params &p, const int32_t *row_scen, int64_t row0, int64_t row_end);
void trig32(dim3 grid, hipStream_t s, const double *h, float *sin_out, float *cos_out, int64_t n);

} // namespace sgl

// CALL(G, WV) for the tile shape (G, WV) of a handle
#define SGL_DISPATCH(G_, WV_, CALL)                                                                                                  \
    do {                                                                                                                             \
        if ((WV_) == 4) { CALL(64, 4); }                                                                                             \
        else if ((WV_) == 2) { CALL(64, 2); }                                                                                        \
        else switch (G_) {                                                                                                           \
            case 4: CALL(4, 1); break;                                                                                               \
            case 8: CALL(8, 1); break;                                                                                               \
            case 16: CALL(16, 1); break;                                                                                             \
            case 32: CALL(32, 1); break;                                                                                             \
            default: CALL(64, 1); break;                                                                                             \
        }                                                                                                                            \
    } while (0)
// CALL(G) for one-wavefront tiles
#define SGL_DISPATCH_G(G_, CALL)                                                                                                     \
    do {                                                                                                                             \
        switch (G_) {                                                                                                                \
        case 4: CALL(4); break;                                                                                                      \
        case 8: CALL(8); break;                                                                                                      \
        case 16: CALL(16); break;                                                                                                    \
        case 32: CALL(32); break;                                                                                                    \
        default: CALL(64); break;                                                                                                    \
        }                                                                                                                            \
    } while (0)
#define SGL_ARGS(a) *(a).p, (a).timestep, (a).n_steps, (a).do_reset, (a).force, (a).actions, (a).tab
