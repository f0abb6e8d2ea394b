// sgym_observers.hpp -- The map and look-ahead observations for ANY entity of a scenario: the observer list kernels.
// Part of the gfx950 device code of the batched rollout engine; included by sgym_device.hpp (in order: every part builds on
// the ones before it), never on its own.
#pragma once

namespace sg {

// ------------------------------------------------------------------------------------------------
// The reference's sensors are per entity: RasterizedMapSensor(entity, ...) rasters the scene in that entity's frame
// (sensor/map.py:136-271), FutureCollisionDetector(entity, horizon) looks ahead along that entity's trajectory
// (sensor/common.py:60-106).  raster_kernel / raster_surface_kernel / future_kernel (sgym_sensors.hpp) answer for the ego of
// each scenario; the kernels here answer for a caller-given list of observers (scenario, slot), one workgroup per observer,
// with the same operation sequences: for the observer (r, ego of r) the bytes are those of the ego kernels.
// ------------------------------------------------------------------------------------------------
struct ObsLayers {
    int32_t code[8]; // layer codes of sg_raster_map: 0 the entity layer, else one SG_LAYER_* bit (by value: no device copy)
};

// All requested layers of observer k = blockIdx.x in one pass over the grid points: the entity layer with the staged corners
// of raster_kernel (the boxes that can reach the grid compacted into LDS, scenarios wider than the workgroup tile by tile),
// the surface layers with ONE rn_layers_at per grid point (observe_kernel).  out [n_obs][n_layers][nh][nw] bytes, every byte
// written; consecutive lanes write consecutive bytes of a plane.  An observer that is not present: all zeros.
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(512) void observers_raster_kernel(Params p, RoadIndex R, int has_road, const int32_t *obs_scen,
                                                                      const int32_t *obs_slot, double width, double height, int nw, int nh,
                                                                      int n_layers, ObsLayers lay, unsigned char *out)
{
    __shared__ double cor[8][512]; // (one thread per entity slot of a tile: 256 threads, 512 for scenarios of more than 256)
    __shared__ double obs_pose[4]; // x, y, sin(theta), cos(theta)
    __shared__ int obs_pres;
    __shared__ int near_n;
    const int k = blockIdx.x, tid = threadIdx.x, nthr = (int)blockDim.x;
    const int r = obs_scen[k], slot = obs_slot[k];
    if (tid == 0) {
        const uint32_t idx = (uint32_t)r * p.EP + (uint32_t)slot;
        const LanePtr dy(p.dyn + (size_t)(idx >> 6) * ((size_t)p.FROWS * 64), (idx & 63) * 8u);
        double s, c;
        sg_sincos(fld(dy, SG_F_POSE + 3) + 3.14159265358979311600e+00 / 2, s, c); // pose[3] + math.pi / 2
        obs_pose[0] = fld(dy, SG_F_POSE + 0); obs_pose[1] = fld(dy, SG_F_POSE + 1);
        obs_pose[2] = s; obs_pose[3] = c;
        obs_pres = fld<uint64_t>(dy, SG_F_PRESENT) != 0;
    }
    __syncthreads();
    const double ex = obs_pose[0], ey = obs_pose[1], s = obs_pose[2], c = obs_pose[3];
    const bool observer_present = obs_pres != 0;
    bool want_entity = false;
    uint32_t want = 0;
    for (int l = 0; l < n_layers; ++l) { want_entity = want_entity || lay.code[l] == 0; want |= (uint32_t)lay.code[l]; }
    const int net = (has_road && R.net_of_scen) ? R.net_of_scen[r] : -1;
    const size_t plane = (size_t)nw * nh;
    unsigned char *o = out + (size_t)k * n_layers * plane;
    // the first tile writes every layer; a later tile (scenarios of more entities than the workgroup has threads) only adds
    // its boxes to the entity planes: a grid point's bytes are this thread's own, written and read back by the same thread
    for (int e0 = 0; e0 == 0 || (want_entity && observer_present && e0 < p.E); e0 += nthr) {
        const int e = e0 + tid;
        if (tid == 0) near_n = 0;
        __syncthreads();
        if (want_entity && observer_present && e < p.E) {
            const uint32_t idx = (uint32_t)r * p.EP + (uint32_t)e;
            const LanePtr st(p.stat + (size_t)(idx >> 6) * (ST_COUNT * 64), (idx & 63) * 8u);
            const LanePtr dy(p.dyn + (size_t)(idx >> 6) * ((size_t)p.FROWS * 64), (idx & 63) * 8u);
            if (fld<uint64_t>(dy, SG_F_PRESENT) != 0) {
                double C[8];
                const double x = fld(dy, SG_F_POSE + 0), y = fld(dy, SG_F_POSE + 1), h = fld(dy, SG_F_POSE + 3);
                double sh, ch;
                sg_sincos(h, sh, ch);
                sg_corners(x, y, sh, ch, fld(st, ST_BW), fld(st, ST_BL), fld(st, ST_BCX), fld(st, ST_BCY), C);
                // only boxes that can reach the grid are tested per cell (the bound of raster_kernel)
                const double reach = 0.5 * (__builtin_fabs(width) + __builtin_fabs(height)) * 1.0000001 + 1e-6;
                double far = 0.0;
#pragma unroll
                for (int m = 1; m < 4; ++m) far = __builtin_fmax(far, __builtin_fabs(C[2 * m] - C[0]) + __builtin_fabs(C[2 * m + 1] - C[1]));
                const double dx = C[0] - ex, dyy = C[1] - ey, lim = reach + far * 1.0000001 + 1e-6 * (1.0 + __builtin_fabs(ex) + __builtin_fabs(ey));
                if (!(dx * dx + dyy * dyy > lim * lim)) { // NaN-safe: keeps the box
                    const int q = atomicAdd(&near_n, 1);
#pragma unroll
                    for (int m = 0; m < 8; ++m) cor[m][q] = C[m];
                }
            }
        }
        __syncthreads();
        const int nn = near_n;
        for (int q = tid; q < nw * nh; q += nthr) {
            bool hit = false;
            uint32_t in = 0u;
            if (observer_present) {
                const int i = q / nw, j = q - i * nw;
                const double x0 = sg_linspace_at(-width / 2, width / 2, nw, j), x1 = sg_linspace_at(-height / 2, height / 2, nh, i);
                const double px = __builtin_fma(x1, -s, x0 * c) + ex, py = __builtin_fma(x1, c, x0 * s) + ey;
                for (int m = 0; m < nn && !hit; ++m) {
                    const double ax = cor[0][m], ay = cor[1][m], bx = cor[2][m], by = cor[3][m];
                    const double cx = cor[4][m], cy = cor[5][m], dx = cor[6][m], dyy = cor[7][m];
                    const double orient = (cx - ax) * (dyy - by) - (cy - ay) * (dx - bx);
                    const double c0 = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
                    const double c1 = (cx - bx) * (py - by) - (cy - by) * (px - bx);
                    const double c2 = (dx - cx) * (py - cy) - (dyy - cy) * (px - cx);
                    const double c3 = (ax - dx) * (py - dyy) - (ay - dyy) * (px - dx);
                    hit = orient > 0 ? (c0 > 0 && c1 > 0 && c2 > 0 && c3 > 0)
                                     : (orient < 0 && c0 < 0 && c1 < 0 && c2 < 0 && c3 < 0);
                }
                if (e0 == 0 && want && has_road) in = rn_layers_at(R, net, want, px, py);
            }
            for (int l = 0; l < n_layers; ++l) {
                unsigned char *b = o + (size_t)l * plane + q;
                if (e0 == 0) *b = lay.code[l] == 0 ? (unsigned char)hit : (unsigned char)((in & (uint32_t)lay.code[l]) != 0);
                else if (hit && lay.code[l] == 0) *b = 1;
            }
        }
        __syncthreads();
    }
}
#endif // SG_UNIT_OBS

// FutureCollisionDetector._step (sensor/common.py:87-106) for observer k = blockIdx.x: future_kernel's two passes with the
// observer's slot where that kernel has the ego's -- pass 1: the observer's corners at every sample time into LDS; pass 2:
// every other (entity, sample) pair against them.  The time base is the clock of the observer's scenario; presence is not
// consulted; a box bit-identical to the observer's never counts (utils.py:59).  out [n_obs] bytes.
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void observers_future_kernel(Params p, const int32_t *obs_scen, const int32_t *obs_slot, double horizon,
                                                                      int n_samples, unsigned char *out)
{
    __shared__ double obs_c[SG_FUT_MAX_SAMPLES][8];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int r = obs_scen[k], slot = obs_slot[k];
    const double start = p.sdyn[r].t, stop = start + horizon;
    const double step = n_samples > 1 ? (stop - start) / (double)(n_samples - 1) : 0.0; // np.linspace
    auto corners_at = [&](int e, int j, double *C) -> bool {
        const uint32_t idx = (uint32_t)r * p.EP + e;
        const LanePtr st(p.stat + (size_t)(idx >> 6) * (ST_COUNT * 64), (idx & 63) * 8u);
        const int64_t meta = fld<int64_t>(st, ST_META);
        if ((int)(meta & 0xff) == SG_KIND_NONE) return false;
        double tj = (double)j * step + start;
        if (n_samples > 1 && j == n_samples - 1) tj = stop;
        double pose[6], s, c;
        own_position_clamped(p.knots + fld<int64_t>(st, ST_KNOT_OFF) * 7, (int)(meta >> 32), tj, pose);
        sg_sincos(pose[3], s, c);
        sg_corners(pose[0], pose[1], s, c, fld(st, ST_BW), fld(st, ST_BL), fld(st, ST_BCX), fld(st, ST_BCY), C);
        return true;
    };
    bool hit = false;
    for (int j0 = 0; j0 < n_samples; j0 += SG_FUT_MAX_SAMPLES) { // more samples than the LDS table holds: in rounds
        const int nj = min(SG_FUT_MAX_SAMPLES, n_samples - j0);
        if (tid < nj) {
            double C[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            corners_at(slot, j0 + tid, C); // (sg_set_observers refuses a slot of SG_KIND_NONE)
#pragma unroll
            for (int m = 0; m < 8; ++m) obs_c[tid][m] = C[m];
        }
        __syncthreads();
        for (int w = tid; w < nj * p.E; w += 256) {
            const int j = w / p.E, e = w - j * p.E;
            double C[8];
            if (e == slot || !corners_at(e, j0 + j, C)) continue;
            double A[8];
            bool same = true;
#pragma unroll
            for (int m = 0; m < 8; ++m) { A[m] = obs_c[j][m]; same = same && (A[m] == C[m]); }
            if (!same && sg_quads_intersect(A, C)) hit = true;
        }
        __syncthreads();
    }
    const int any = __syncthreads_or(hit);
    if (tid == 0) out[k] = (unsigned char)(any != 0);
}
#endif // SG_UNIT_OBS

} // namespace sg
