// sgym_observers.hpp -- The map and look-ahead observations: one raster kernel and one look-ahead kernel for the ego of every
// scenario and for a caller-given list of observers (any entity).
// Part of the gfx950 device code of the batched rollout engine; included by sgym_device.hpp (in order: every part builds on
// the ones before it), never on its own.
#pragma once

namespace sg {

// ------------------------------------------------------------------------------------------------
// The reference's sensors are per entity: RasterizedMapSensor(entity, ...) rasters the scene in that entity's frame
// (sensor/map.py:120-271), FutureCollisionDetector(entity, horizon) looks ahead along that entity's trajectory
// (sensor/common.py:60-106), SURVEY 8f N2.  One workgroup per observer k = blockIdx.x: (obs_scen[k], obs_slot[k]) of a list, or
// -- without a list (obs_scen == nullptr) -- the ego of scenario k.  fp64 throughout, the operation sequences of the oracle
// (np.linspace / numpy matmul arithmetic as probed there).
// ------------------------------------------------------------------------------------------------
struct ObsLayers {
    int32_t code[8]; // layer codes of sg_raster_map: 0 the entity layer, else one SG_LAYER_* bit (by value: no device copy)
};

// the observer's frame, staged in LDS by one thread: position, sin / cos of heading + pi/2, presence
struct ObsFrame {
    double x, y, s, c;
    int present; // (the reference sensor needs state.poses[entity]: an observer that is not in the scene sees nothing)
};

__device__ __forceinline__ void obs_stage_frame(const Params &p, int r, int slot, ObsFrame &f)
{
    const uint32_t idx = (uint32_t)r * p.EP + (uint32_t)slot;
    const LanePtr dy(p.dyn + (size_t)(idx >> 6) * ((size_t)p.FROWS * 64), (idx & 63) * 8u);
    double s, c;
    sg_sincos(fld(dy, SG_F_POSE + 3) + 3.14159265358979311600e+00 / 2, s, c); // pose[3] + math.pi / 2
    f.x = fld(dy, SG_F_POSE + 0); f.y = fld(dy, SG_F_POSE + 1);
    f.s = s; f.c = c;
    f.present = fld<uint64_t>(dy, SG_F_PRESENT) != 0;
}

__device__ __forceinline__ double sg_linspace_at(double start, double stop, int n, int j)
{
    if (n > 1 && j == n - 1) return stop;
    const double step = n > 1 ? (stop - start) / (double)(n - 1) : 0.0;
    return (double)j * step + start;
}

// grid point q of the nh x nw grid (row i = q / nw along the height) in world coordinates: the frame rotated by heading + pi/2
__device__ __forceinline__ void obs_grid_point(double ex, double ey, double s, double c, double width, double height, int nw, int nh, int q,
                                               double &px, double &py)
{
    const int i = q / nw, j = q - i * nw;
    const double x0 = sg_linspace_at(-width / 2, width / 2, nw, j), x1 = sg_linspace_at(-height / 2, height / 2, nh, i);
    px = __builtin_fma(x1, -s, x0 * c) + ex;
    py = __builtin_fma(x1, c, x0 * s) + ey;
}

// Entity e of scenario r, if it is present and its box can reach the grid around (ex, ey): its corners go into the next free
// column of cor (*near_n counts them).  Every grid point lies within `reach` of the observer (the grid's half diagonal,
// generously rounded up), every point of a box within the largest corner distance of its first corner.
__device__ __forceinline__ void obs_stage_box(const Params &p, int r, int e, double ex, double ey, double width, double height,
                                              double (&cor)[8][512], int *near_n)
{
    const uint32_t idx = (uint32_t)r * p.EP + (uint32_t)e;
    const LanePtr st(p.stat + (size_t)(idx >> 6) * (ST_COUNT * 64), (idx & 63) * 8u);
    const LanePtr dy(p.dyn + (size_t)(idx >> 6) * ((size_t)p.FROWS * 64), (idx & 63) * 8u);
    if (fld<uint64_t>(dy, SG_F_PRESENT) == 0) return;
    double C[8];
    const double x = fld(dy, SG_F_POSE + 0), y = fld(dy, SG_F_POSE + 1), h = fld(dy, SG_F_POSE + 3);
    double sh, ch;
    sg_sincos(h, sh, ch);
    sg_corners(x, y, sh, ch, fld(st, ST_BW), fld(st, ST_BL), fld(st, ST_BCX), fld(st, ST_BCY), C);
    const double reach = 0.5 * (__builtin_fabs(width) + __builtin_fabs(height)) * 1.0000001 + 1e-6;
    double far = 0.0;
#pragma unroll
    for (int m = 1; m < 4; ++m) far = __builtin_fmax(far, __builtin_fabs(C[2 * m] - C[0]) + __builtin_fabs(C[2 * m + 1] - C[1]));
    const double dx = C[0] - ex, dyy = C[1] - ey, lim = reach + far * 1.0000001 + 1e-6 * (1.0 + __builtin_fabs(ex) + __builtin_fabs(ey));
    if (dx * dx + dyy * dyy > lim * lim) return; // (NaN-safe: keeps the box)
    const int q = atomicAdd(near_n, 1);
#pragma unroll
    for (int m = 0; m < 8; ++m) cor[m][q] = C[m];
}

// does (px, py) lie strictly inside one of the nn staged boxes (either winding; a degenerate box contains nothing)
__device__ __forceinline__ bool obs_in_staged_boxes(const double (&cor)[8][512], int nn, double px, double py)
{
    bool hit = false;
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
    return hit;
}

// All requested layers of observer k in one pass over the grid points.  The entity layer: cell = 1 iff the grid point lies
// strictly inside the box of a present entity (the observer included); the boxes that can reach the grid are compacted into
// LDS once per tile of blockDim.x entity slots (256 threads, 512 for scenarios of more than 256), scenarios wider than that
// go tile by tile.  The surface layers: ONE rn_layers_at per grid point for all of them; empty without road networks
// (has_road == 0).  Layer l of observer k is the plane out + k * stride + l * nh * nw; every byte of it is written, consecutive
// lanes write consecutive bytes.  An observer that is not present: all zeros.
// TICK (sg_tick's one observation launch; no list; scenarios of at most one tile): also flags[r] = the SG_TERM_* bits of the
// state, as terminal_flags_kernel gives them.
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
template <bool TICK>
static __global__ __launch_bounds__(512) void map_raster_kernel(Params p, RoadIndex R, int has_road, const int32_t *obs_scen,
                                                                const int32_t *obs_slot, double width, double height, int nw, int nh,
                                                                int n_layers, ObsLayers lay, unsigned char *out, int64_t stride,
                                                                uint32_t *flags /*[R], TICK only*/)
{
    __shared__ double cor[8][512];
    __shared__ ObsFrame frame;
    __shared__ int near_n;
    const int k = blockIdx.x, tid = threadIdx.x, nthr = (int)blockDim.x;
    const int r = obs_scen ? obs_scen[k] : k, slot = obs_scen ? obs_slot[k] : p.sstat[k].ego;
    if (tid == 0) obs_stage_frame(p, r, slot, frame);
    if constexpr (TICK) {
        const int W = p.FROWS - SG_F_COLL;
        bool any_coll = false, e0_present = false, e0_coll = false;
        double x0 = 0.0, y0 = 0.0;
        for (int e = tid; e < p.E; e += nthr) {
            const uint32_t idx = (uint32_t)r * p.EP + (uint32_t)e;
            const LanePtr dy(p.dyn + (size_t)(idx >> 6) * ((size_t)p.FROWS * 64), (idx & 63) * 8u);
            const bool present = fld<uint64_t>(dy, SG_F_PRESENT) != 0;
            bool mine = false;
            for (int w = 0; w < W; ++w) mine = mine || fld<uint64_t>(dy, SG_F_COLL + w) != 0;
            any_coll = any_coll || (present && mine);
            if (e == 0) { e0_present = present; e0_coll = mine; x0 = fld(dy, SG_F_POSE + 0); y0 = fld(dy, SG_F_POSE + 1); }
        }
        const int any = __syncthreads_or(any_coll);
        if (tid == 0) flags[r] = sg_terminal_bits_of_entity0(p, r, e0_present, e0_coll, x0, y0) | (any ? SG_TERM_COLLISION : 0u);
    } else {
        __syncthreads();
    }
    const double ex = frame.x, ey = frame.y, s = frame.s, c = frame.c;
    const bool observer_present = frame.present != 0;
    bool want_entity = false;
    uint32_t want = 0;
    for (int l = 0; l < n_layers; ++l) { want_entity = want_entity || lay.code[l] == 0; want |= (uint32_t)lay.code[l]; }
    const int net = (has_road && R.net_of_scen) ? R.net_of_scen[r] : -1;
    const size_t plane = (size_t)nw * nh;
    unsigned char *o = out + (size_t)k * stride;
    // the first tile writes every layer; a later tile only adds its boxes to the entity planes: a grid point's bytes are this
    // thread's own, written and read back by the same thread
    for (int e0 = 0; e0 == 0 || (want_entity && observer_present && e0 < p.E); e0 += nthr) {
        if (tid == 0) near_n = 0;
        __syncthreads();
        if (want_entity && observer_present && e0 + tid < p.E) obs_stage_box(p, r, e0 + tid, ex, ey, width, height, cor, &near_n);
        __syncthreads();
        const int nn = near_n;
        for (int q = tid; q < nw * nh; q += nthr) {
            bool hit = false;
            uint32_t in = 0u;
            if (observer_present) {
                double px, py;
                obs_grid_point(ex, ey, s, c, width, height, nw, nh, q, px, py);
                hit = obs_in_staged_boxes(cor, nn, px, py);
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

// FutureCollisionDetector._step (sensor/common.py:87-106) for observer k: does its box, moved along its trajectory to n sample
// times in [t, t + horizon] (np.linspace), overlap any other entity's box at that entity's own trajectory position (clamped
// outside the trajectory)?  The (entity, sample) pairs are spread over the 256 threads (the binary searches over the knots are
// chains of dependent loads: 10 samples one after the other per entity thread took 250 us for 4096 x 64).  Pass 1: the
// observer's corners at every sample time into LDS; pass 2: every other pair against them, the exact fp64 predicate.  The time
// base is the clock of the observer's scenario; presence is not consulted; a box bit-identical to the observer's never counts
// (utils.py:59).  out [n observers] bytes.
#define SG_FUT_MAX_SAMPLES 64
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void look_ahead_kernel(Params p, const int32_t *obs_scen, const int32_t *obs_slot, double horizon,
                                                                int n_samples, unsigned char *out)
{
    __shared__ double obs_c[SG_FUT_MAX_SAMPLES][8];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int r = obs_scen ? obs_scen[k] : k, slot = obs_scen ? obs_slot[k] : p.sstat[k].ego;
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
            corners_at(slot, j0 + tid, C); // (an ego is an entity; sg_set_observers refuses a slot of SG_KIND_NONE)
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
