// k_obs.hip -- map_raster_kernel / look_ahead_kernel / nearest_kernel / lane_observation_kernel / range_scan_kernel /
// entity_status_kernel / route_observation_kernel / time_to_collision_kernel / surface_scan_kernel / pose_history_kernel: the map,
// look-ahead, nearest-entity, lane-frame, range-scan, route, time-to-collision, surface-scan and pose-history observations and the episode status of the ego
// of every scenario or of a list of observers (scenario, slot), any entity of its scenario (sgym_observers.hpp).
#define SG_UNIT_OBS
#include "sgym_launch.hpp"

namespace sgl {
void map_raster(hipStream_t s, const sg::Params &p, const sg::RoadIndex &R, bool has_road, const int32_t *scen, const int32_t *slot, int64_t n,
                double width, double height, int nw, int nh, int n_layers, const int32_t *layers, unsigned char *out, int64_t stride,
                uint32_t *flags)
{
    if (n <= 0) return;
    sg::ObsLayers lay{};
    for (int k = 0; k < n_layers && k < 8; ++k) lay.code[k] = layers[k];
    const dim3 grid((unsigned)n), block(p.EP > 256 ? 512 : 256);
    if (flags)
        sg::map_raster_kernel<true><<<grid, block, 0, s>>>(p, R, has_road ? 1 : 0, nullptr, nullptr, width, height, nw, nh, n_layers, lay, out, stride, flags);
    else
        sg::map_raster_kernel<false><<<grid, block, 0, s>>>(p, R, has_road ? 1 : 0, scen, slot, width, height, nw, nh, n_layers, lay, out, stride, nullptr);
}

void look_ahead(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, double horizon, int n_samples,
                unsigned char *out)
{
    if (n <= 0) return;
    sg::look_ahead_kernel<<<dim3((unsigned)n), dim3(256), 0, s>>>(p, scen, slot, horizon, n_samples, out);
}

void nearest(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, int k, double radius, double *feat,
             int32_t *slots, int32_t *count)
{
    if (n <= 0) return;
    const double r2 = radius * radius; // (+inf for an infinite radius: every finite distance passes)
    const dim3 per_wave((unsigned)((n + 3) / 4)), block(256);
    if (p.E > 512) sg::nearest_kernel<0><<<dim3((unsigned)n), block, 0, s>>>(p, scen, slot, n, k, r2, feat, slots, count);
    else if (p.E > 256) sg::nearest_kernel<8><<<per_wave, block, 0, s>>>(p, scen, slot, n, k, r2, feat, slots, count);
    else if (p.E > 128) sg::nearest_kernel<4><<<per_wave, block, 0, s>>>(p, scen, slot, n, k, r2, feat, slots, count);
    else if (p.E > 64) sg::nearest_kernel<2><<<per_wave, block, 0, s>>>(p, scen, slot, n, k, r2, feat, slots, count);
    else sg::nearest_kernel<1><<<per_wave, block, 0, s>>>(p, scen, slot, n, k, r2, feat, slots, count);
}

void pose_history(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, int n_samples, int stride, int k,
                  double radius, double *feat, int32_t *slots, int32_t *count)
{
    if (n <= 0) return;
    const double r2 = radius * radius; // (+inf for an infinite radius: every finite distance passes)
    const dim3 per_wave((unsigned)((n + 3) / 4)), block(256);
    if (p.E > 512) sg::pose_history_kernel<0><<<dim3((unsigned)n), block, 0, s>>>(p, scen, slot, n, n_samples, stride, k, r2, feat, slots, count);
    else if (p.E > 256) sg::pose_history_kernel<8><<<per_wave, block, 0, s>>>(p, scen, slot, n, n_samples, stride, k, r2, feat, slots, count);
    else if (p.E > 128) sg::pose_history_kernel<4><<<per_wave, block, 0, s>>>(p, scen, slot, n, n_samples, stride, k, r2, feat, slots, count);
    else if (p.E > 64) sg::pose_history_kernel<2><<<per_wave, block, 0, s>>>(p, scen, slot, n, n_samples, stride, k, r2, feat, slots, count);
    else sg::pose_history_kernel<1><<<per_wave, block, 0, s>>>(p, scen, slot, n, n_samples, stride, k, r2, feat, slots, count);
}

void lane_observation(hipStream_t s, const sg::Params &p, const sg::LaneIndex &L, const int32_t *scen, const int32_t *slot, int64_t n, int k,
                      int n_ahead, double spacing, double radius, double *feat, int32_t *lanes, int32_t *count)
{
    if (n <= 0) return;
    const double r2 = radius * radius; // (+inf for an infinite radius: every finite distance passes)
    sg::lane_observation_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s>>>(p, L, scen, slot, n, k, n_ahead, spacing, r2, feat, lanes, count);
}

void range_scan(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, int n_rays, double angle0, double dangle,
                double max_range, double *feat, int32_t *slots, int32_t *hits)
{
    if (n <= 0) return;
    sg::range_scan_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s>>>(p, scen, slot, n, n_rays, angle0, dangle, max_range, feat, slots, hits);
}

void entity_status(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, uint32_t *flags, int32_t *info,
                   double *feat)
{
    if (n <= 0) return;
    sg::entity_status_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s>>>(p, scen, slot, n, flags, info, feat);
}

void route_observation(hipStream_t s, const sg::Params &p, const sg::RouteIndex &P, const int32_t *scen, const int32_t *slot, int64_t n,
                       int n_ahead, double spacing, double *feat, int32_t *info)
{
    if (n <= 0) return;
    sg::route_observation_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s>>>(p, P, scen, slot, n, n_ahead, spacing, feat, info);
}

void time_to_collision(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, double horizon, double *feat,
                       int32_t *info)
{
    if (n <= 0) return;
    sg::time_to_collision_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s>>>(p, scen, slot, n, horizon, feat, info);
}

void surface_scan(hipStream_t s, const sg::Params &p, const int32_t *scen, const int32_t *slot, int64_t n, int n_layers, const int32_t *layers,
                  int n_rays, double angle0, double dangle, double step, int n_steps, int n_refine, double *feat, unsigned char *flags,
                  int32_t *hits)
{
    if (n <= 0) return;
    sg::SurfLayers lay{};
    for (int k = 0; k < n_layers && k < 8; ++k) lay.bit[k] = (uint32_t)layers[k];
    sg::surface_scan_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s>>>(p, scen, slot, n, lay, n_layers, n_rays, angle0, dangle, step, n_steps,
                                                                                n_refine, feat, flags, hits);
}
} // namespace sgl
