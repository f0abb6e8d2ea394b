// sgym_observers.hpp -- The map, look-ahead, nearest-entity, lane-frame, range-scan, route, time-to-collision, surface-scan and pose-history observations and the
// entity status: one kernel each for the ego of every scenario and for a caller-given list of observers (any entity).
// Part of the gfx950 device code of the batched rollout engine; included by sgym_device.hpp (in order: every part builds on
// the ones before it), never on its own.
#pragma once

namespace sg {

// the first dynamic / static row of padded entity index idx = r * EP + slot: field f is at [f * 64]
__device__ __forceinline__ const double *entity_dyn(const Params &p, uint32_t idx) { return p.dyn + (size_t)(idx >> 6) * ((size_t)p.FROWS * 64) + (idx & 63); }
__device__ __forceinline__ const double *entity_stat(const Params &p, uint32_t idx) { return p.stat + (size_t)(idx >> 6) * (ST_COUNT * 64) + (idx & 63); }
__device__ __forceinline__ bool entity_present(const double *dyn) { return reinterpret_cast<const uint64_t *>(dyn)[SG_F_PRESENT * 64] != 0; }

// ------------------------------------------------------------------------------------------------
// The reference's sensors are per entity: RasterizedMapSensor(entity, ...) rasters the scene in that entity's frame
// (sensor/map.py:120-271), FutureCollisionDetector(entity, horizon) looks ahead along that entity's trajectory
// (sensor/common.py:60-106), SURVEY 8f N2.  One workgroup per observer k = blockIdx.x, listed or ego as in observer_of.
// fp64 throughout, the operation sequences of the oracle (np.linspace / numpy matmul arithmetic as probed there).
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
    const double *dy = entity_dyn(p, (uint32_t)r * p.EP + (uint32_t)slot);
    double s, c;
    sg_sincos(dy[(SG_F_POSE + 3) * 64] + 3.14159265358979311600e+00 / 2, s, c); // pose[3] + math.pi / 2
    f.x = dy[(SG_F_POSE + 0) * 64]; f.y = dy[(SG_F_POSE + 1) * 64];
    f.s = s; f.c = c;
    f.present = entity_present(dy);
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
    const double *st = entity_stat(p, idx), *dy = entity_dyn(p, idx);
    if (!entity_present(dy)) return;
    double C[8];
    const double x = dy[(SG_F_POSE + 0) * 64], y = dy[(SG_F_POSE + 1) * 64], h = dy[(SG_F_POSE + 3) * 64];
    double sh, ch;
    sg_sincos(h, sh, ch);
    sg_corners(x, y, sh, ch, st[ST_BW * 64], st[ST_BL * 64], st[ST_BCX * 64], st[ST_BCY * 64], C);
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
            const double *dy = entity_dyn(p, (uint32_t)r * p.EP + (uint32_t)e);
            const bool present = entity_present(dy);
            bool mine = false;
            for (int w = 0; w < W; ++w) mine = mine || reinterpret_cast<const uint64_t *>(dy)[(SG_F_COLL + w) * 64] != 0;
            any_coll = any_coll || (present && mine);
            if (e == 0) { e0_present = present; e0_coll = mine; x0 = dy[(SG_F_POSE + 0) * 64]; y0 = dy[(SG_F_POSE + 1) * 64]; }
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
        const double *st = entity_stat(p, (uint32_t)r * p.EP + e);
        const int64_t *sti = reinterpret_cast<const int64_t *>(st);
        const int64_t meta = sti[ST_META * 64];
        if ((int)(meta & 0xff) == SG_KIND_NONE) return false;
        double tj = (double)j * step + start;
        if (n_samples > 1 && j == n_samples - 1) tj = stop;
        double pose[6], s, c;
        own_position_clamped(p.knots + sti[ST_KNOT_OFF * 64] * 7, (int)(meta >> 32), tj, pose);
        sg_sincos(pose[3], s, c);
        sg_corners(pose[0], pose[1], s, c, st[ST_BW * 64], st[ST_BL * 64], st[ST_BCX * 64], st[ST_BCY * 64], C);
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

// ------------------------------------------------------------------------------------------------
// The observer and its scenario, as the kernels below and driver_policy_kernel (sgym_policy.hpp) read them: one wavefront per
// observer in workgroups of 256.  What belongs to the observer alone is the same in every lane: each lane loads and computes
// it for itself (one address per load, one sg_sincos), which costs no more than staging it would, and what a kernel does not
// use of it falls to the compiler.  The scenario's slots go by in blocks of 64, lane = entity.
// ------------------------------------------------------------------------------------------------
// the thread's lane and its wavefront's item o = 4 * block + wave_index() (whole_group: o = block, the four wavefronts share it);
// false: no item o < n -- for the whole wavefront, or workgroup
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ bool wave_item(int64_t n, int &lane, int64_t &o, bool whole_group = false)
{
    lane = threadIdx.x & 63;
    o = whole_group ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave_index();
    return o < n;
}

// the observer: scenario, slot, position, velocity, sin / cos of its heading, presence (the reference's sensors need
// state.poses[entity]: an observer that is not in the scene sees nothing); to_frame: a world vector in the observer's frame
struct Observer {
    double x, y, vx, vy, s, c;
    int r, slot, present;
    __device__ __forceinline__ void to_frame(double X, double Y, double &fx, double &fy) const { fx = X * c + Y * s; fy = Y * c - X * s; }
};

__device__ __forceinline__ Observer observer_at(const Params &p, int r, int slot)
{
    Observer f;
    f.r = r; f.slot = slot;
    const double *d = entity_dyn(p, (uint32_t)r * p.EP + (uint32_t)slot);
    f.present = entity_present(d);
    f.x = d[(SG_F_POSE + 0) * 64]; f.y = d[(SG_F_POSE + 1) * 64];
    f.vx = d[(SG_F_VEL + 0) * 64]; f.vy = d[(SG_F_VEL + 1) * 64];
    sg_sincos(d[(SG_F_POSE + 3) * 64], f.s, f.c);
    return f;
}

// observer o of a list: (obs_scen[o], obs_slot[o]), or -- without a list (obs_scen == nullptr) -- the ego of scenario o
__device__ __forceinline__ Observer observer_of(const Params &p, const int32_t *obs_scen, const int32_t *obs_slot, int64_t o)
{
    return observer_at(p, obs_scen ? obs_scen[o] : (int)o, obs_scen ? obs_slot[o] : p.sstat[o].ego);
}

// Slot e of the observer's scenario: its rows, whether it is an entity other than the observer, and (a load) whether it is in
// the scene.  A lane without a slot (e >= E) reads the observer's own rows, which are there, as e == f.slot does: other == false.
struct ObservedSlot {
    const double *dyn, *stat; // entity_dyn / entity_stat
    bool other;
    __device__ __forceinline__ bool present() const { return entity_present(dyn); }
};

__device__ __forceinline__ ObservedSlot observed_slot(const Params &p, const Observer &f, int e)
{
    const bool other = e < p.E && e != f.slot;
    const uint32_t idx = (uint32_t)f.r * p.EP + (uint32_t)(other ? e : f.slot);
    return {entity_dyn(p, idx), entity_stat(p, idx), other};
}

// ------------------------------------------------------------------------------------------------
// The vector observation: the k nearest entities around an observer, in the observer's frame (no counterpart in the
// reference, whose State.get_entities_in_radius answers for one scenario on the host).  Candidates are the other present
// entities of the observer's scenario with a finite squared distance d2 = dx * dx + dy * dy <= radius * radius (plain fp64,
// unfused); the order is ascending (d2, slot), the key of the selection d2 as a 64-bit integer (KEY_NONE, sgym_polyline.hpp).
// ------------------------------------------------------------------------------------------------
#define SG_NEAR_MAX_K 32

// the key of slot e of the observer's scenario; KEY_NONE for the observer itself and for a lane without a slot
__device__ __forceinline__ uint64_t near_key(const Params &p, const Observer &f, int e, double r2)
{
    const ObservedSlot q = observed_slot(p, f, e);
    const bool present = q.present();
    const double dx = q.dyn[(SG_F_POSE + 0) * 64] - f.x, dy = q.dyn[(SG_F_POSE + 1) * 64] - f.y;
    const double d2 = dx * dx + dy * dy;
    const bool in = q.other && present && d2 <= r2 && d2 < __builtin_inf(); // (a NaN fails both)
    return in ? (uint64_t)__double_as_longlong(d2) : KEY_NONE;
}

// k rounds over the N register entries of every lane: the wavefront's minimum, which its owner retires (slots are unique;
// an entry that holds nothing has slot INDEX_NONE).  Lane j returns the slot of round j, -1 once the candidates ran out.
template <int N>
__device__ __forceinline__ int near_select(uint64_t (&key)[N], const int (&slot)[N], int k, int lane)
{
    int mine = -1;
    for (int j = 0; j < k; ++j) {
        uint64_t bk = KEY_NONE;
        int bs = INDEX_NONE;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const bool take = key[i] < bk || (key[i] == bk && slot[i] < bs);
            bk = take ? key[i] : bk;
            bs = take ? slot[i] : bs;
        }
        wave_min(bk, bs);
        if (bk == KEY_NONE) break; // (the same in every lane)
#pragma unroll
        for (int i = 0; i < N; ++i) key[i] = slot[i] == bs ? KEY_NONE : key[i];
        if (lane == j) mine = bs;
    }
    return mine;
}

// row `lane` of observer o: the eight features of neighbour nb (zeros for nb < 0), its slot, and the observer's count
__device__ __forceinline__ void near_store(const Params &p, const Observer &f, int64_t o, int k, int lane, int nb, int total,
                                           double *feat, int32_t *slots, int32_t *count)
{
    if (lane == 0 && count) count[o] = total;
    if (lane >= k) return;
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (nb >= 0) {
        const uint32_t idx = (uint32_t)f.r * p.EP + (uint32_t)nb;
        const double *d = entity_dyn(p, idx), *st = entity_stat(p, idx);
        double se, ce;
        sg_sincos(d[(SG_F_POSE + 3) * 64], se, ce);
        f.to_frame(d[(SG_F_POSE + 0) * 64] - f.x, d[(SG_F_POSE + 1) * 64] - f.y, v[0], v[1]);
        f.to_frame(ce, se, v[2], v[3]);
        f.to_frame(d[(SG_F_VEL + 0) * 64] - f.vx, d[(SG_F_VEL + 1) * 64] - f.vy, v[4], v[5]);
        v[6] = st[ST_BL * 64];
        v[7] = st[ST_BW * 64];
    }
    double *row = feat + ((size_t)o * k + lane) * 8; // (64 bytes per lane, consecutive lanes consecutive rows)
#pragma unroll
    for (int m = 0; m < 8; ++m) row[m] = v[m];
    if (slots) slots[(size_t)o * k + lane] = nb;
}

// Observer o < n: observer_of.  feat [n][k][8] fp64, slots
// [n][k] (-1 behind the last neighbour; may be nullptr), count [n] (candidates within the radius, it may exceed k; -1 for an
// observer that is not present, whose rows are zeros; may be nullptr).  Every byte of the three is written.  1 <= k <= 32.
// NB > 0 (scenarios of at most NB * 64 <= 512 entities): one wavefront per observer, four observers per workgroup.  Lane l owns
// the slots l, l + 64, ... of the scenario's NB blocks -- a load is one 512-byte row per block -- and keeps their keys in
// registers; the selection is near_select; then lane j computes and stores the features of neighbour j.
// NB == 0 (the wide path, up to 16384 entities): one workgroup of four wavefronts per observer.  Wavefront w takes the
// blocks w, w + 4, ...: round j rescans them for the smallest (key, slot) above the one round j - 1 found (the keys of up to 64
// slots per lane do not fit registers; the rows come from the caches).  The <= 4 * k finalists go through LDS to wavefront 0,
// which selects among them as the narrow path does.
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
// The selection of nearest_kernel<NB> below, which pose_history_kernel<NB> shares: lane j returns the slot of neighbour j of the
// present observer f (-1 behind the last), `total` the candidates within the radius.  NB == 0: every wavefront of the workgroup
// calls it (it holds a barrier); the answers are wavefront 0's alone, the others return -1.
template <int NB>
__device__ __forceinline__ int near_neighbours(const Params &p, const Observer &f, int k, double r2, int lane, int w, int &total)
{
    if constexpr (NB > 0) {
        uint64_t key[NB];
        int slot[NB];
        total = 0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            slot[j] = lane + 64 * j;
            key[j] = near_key(p, f, slot[j], r2);
            total += __popcll(__ballot(key[j] != KEY_NONE));
        }
        return near_select<NB>(key, slot, k, lane);
    } else {
        __shared__ uint64_t fin_key[4 * SG_NEAR_MAX_K];
        __shared__ int fin_slot[4 * SG_NEAR_MAX_K];
        __shared__ int fin_total[4];
        const int n_blocks = (p.E + 63) >> 6;
        uint64_t last_key = 0, my_key = KEY_NONE;
        int last_slot = -1, my_slot = INDEX_NONE;
        total = 0;
        for (int j = 0; j < k; ++j) {
            uint64_t bk = KEY_NONE;
            int bs = INDEX_NONE;
            for (int b = w; b < n_blocks; b += 4) {
                const int e = b * 64 + lane;
                const uint64_t ke = near_key(p, f, e, r2);
                if (j == 0) total += __popcll(__ballot(ke != KEY_NONE));
                const bool after = ke > last_key || (ke == last_key && e > last_slot);
                const bool take = after && (ke < bk || (ke == bk && e < bs));
                bk = take ? ke : bk;
                bs = take ? e : bs;
            }
            wave_min(bk, bs);
            if (bk == KEY_NONE) break; // (the same in every lane: the stripe has run out)
            if (lane == j) { my_key = bk; my_slot = bs; }
            last_key = bk; last_slot = bs;
        }
        if (lane < SG_NEAR_MAX_K) { fin_key[w * SG_NEAR_MAX_K + lane] = my_key; fin_slot[w * SG_NEAR_MAX_K + lane] = my_slot; }
        if (lane == 0) fin_total[w] = total;
        __syncthreads();
        if (w != 0) return -1;
        uint64_t key[2] = {fin_key[lane], fin_key[lane + 64]};
        const int slot[2] = {fin_slot[lane], fin_slot[lane + 64]};
        total = fin_total[0] + fin_total[1] + fin_total[2] + fin_total[3];
        return near_select<2>(key, slot, k, lane);
    }
}

template <int NB>
static __global__ __launch_bounds__(256) void nearest_kernel(Params p, const int32_t *obs_scen, const int32_t *obs_slot, int64_t n, int k,
                                                             double r2, double *feat, int32_t *slots, int32_t *count)
{
    int lane; int64_t o;
    if (!wave_item(n, lane, o, NB == 0)) return; // (NB > 0: the whole wavefront, which meets no barrier)
    const int w = wave_index();
    const Observer f = observer_of(p, obs_scen, obs_slot, o);
    if (!f.present) { // (the whole workgroup on the wide path)
        if (NB || w == 0) near_store(p, f, o, k, lane, -1, -1, feat, slots, count);
        return;
    }
    int total;
    const int nb = near_neighbours<NB>(p, f, k, r2, lane, w, total);
    if (NB == 0 && w != 0) return;
    near_store(p, f, o, k, lane, nb, total, feat, slots, count);
}
#endif // SG_UNIT_OBS

// ------------------------------------------------------------------------------------------------
// The lane-frame vector observation: where an observer sits relative to the k nearest lane centre lines of its scenario's
// network, and where those lines go next (no counterpart in the reference, which only stores Lane.center and the successor
// ids).  The definition is in include/sgym.h at sg_lane_observation; the rows below are built by sg_set_lanes (h_road.hip).
// Segments (LaneSeg rows, sgym_polyline.hpp) are listed lane by lane, so a lane's segments are consecutive and segment order is
// lane order.  (SG_LANE_MAX_K, SG_LANE_MAX_AHEAD, SG_LANE_MAX_HOPS: include/sgym.h.)
// ------------------------------------------------------------------------------------------------

struct LaneRow {      // one lane
    double total;           // its length: cum + len of its last segment (0 without segments)
    int32_t seg0, seg1;     // its segments [seg0, seg1)
    int32_t succ0, succ1;   // its successors succ[succ0 .. succ1): lane indices over all networks, ascending
};
struct LaneNet {      // one network
    int32_t lane0, lane1, seg0, seg1; // its lanes and (all of) their segments
};
struct LaneIndex {    // device pointers, by value; seg == nullptr: no lanes set
    const LaneSeg *seg;
    const LaneRow *lane;
    const int32_t *succ;
    const LaneNet *net;
    const int32_t *net_of_scen; // the list of sg_set_road_networks
};

// the centre-line point at arclength `target` from the start of lane q, walked through the lowest-index successors that
// have segments
__device__ __forceinline__ void lane_point_ahead(const LaneIndex &L, int q, double target, double &x, double &y)
{
    LaneRow row = L.lane[q];
    for (int hops = 0; target > row.total && hops < SG_LANE_MAX_HOPS; ++hops) {
        int next = -1;
        for (int m = row.succ0; m < row.succ1 && next < 0; ++m) {
            const int cand = L.succ[m];
            if (L.lane[cand].seg1 > L.lane[cand].seg0) next = cand;
        }
        if (next < 0) break;
        target -= row.total;
        row = L.lane[next];
    }
    polyline_point_at(L.seg, row.seg0, row.seg1, row.total, target, x, y); // (beyond the end of the walk: the lane's last point)
}

// Observer o < n: observer_of; feat [n][k][6 + 2 * n_ahead], lanes [n][k] (may be nullptr), count [n] (may be nullptr),
// every byte written.  One wavefront per observer, four observers per workgroup, no LDS, no atomics.
// Selection: k rounds; in each the wavefront's lanes stride over the network's segment rows (a load is 64 consecutive 80-byte
// rows), skip the segments of the road lanes chosen so far -- at most eight ids, the same in every lane of the wavefront --
// and keep the smallest (d2 bits, segment index); wave_min makes it the wavefront's.  A rescan per round rather than a
// table of per-road-lane minima in LDS: a network has no bound on its lanes, so the table would need a second path for
// the networks that do not fit, and k times the segment tests of the largest committed network (11,040 points) is below the
// launch overhead of the call.  Round 0 also counts the candidates: a segment within the radius counts for its road lane iff no
// earlier segment of that lane is within the radius -- the 64 segments of one stride step are consecutive, so that is a ballot
// and the lane counted last.
// Then item j * (n_ahead + 1) + m of the wavefront is feature group m of row j: group 0 the six scalars of the best segment,
// group m >= 1 the m-th point ahead.
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void lane_observation_kernel(Params p, LaneIndex L, const int32_t *obs_scen, const int32_t *obs_slot,
                                                                      int64_t n, int k, int n_ahead, double spacing, double r2, double *feat,
                                                                      int32_t *lanes, int32_t *count)
{
    int lane; int64_t o;
    if (!wave_item(n, lane, o)) return; // (the whole wavefront, which meets no barrier)
    const Observer f = observer_of(p, obs_scen, obs_slot, o);
    const int net = (f.present && L.seg) ? L.net_of_scen[f.r] : -1;
    int total = f.present ? 0 : -1, found = 0;
    int mine = 0; // lane j: the best segment of row j
    if (net >= 0) {
        const LaneNet N = L.net[net];
        int ch[SG_LANE_MAX_K]; // the road lanes chosen so far (wavefront-uniform; registers: only ever indexed by unrolled loops)
#pragma unroll
        for (int m = 0; m < SG_LANE_MAX_K; ++m) ch[m] = -1;
        int counted = -1; // round 0: the last road lane counted
        for (int j = 0; j < k; ++j) {
            uint64_t bk = KEY_NONE;
            int bs = INDEX_NONE;
            for (int i0 = N.seg0; i0 < N.seg1; i0 += 64) { // (uniform trip count: the ballot below is the whole wavefront's)
                const int i = i0 + lane;
                const LaneSeg g = L.seg[min(i, N.seg1 - 1)];
                double dx, dy, t;
                const double d2 = lane_project(g, f.x, f.y, dx, dy, t);
                bool in = i < N.seg1 && d2 <= r2 && d2 < __builtin_inf(); // (a NaN fails both)
                if (j == 0) {
                    const uint64_t q = __ballot(in);
                    const int run = max(g.first - i0, 0); // where this road lane's segments start within the step
                    const uint64_t before = q & ((1ull << lane) - 1) & ~((1ull << run) - 1);
                    total += __popcll(__ballot(in && before == 0 && g.lane != counted));
                    if (q) counted = __shfl(g.lane, 63 - __clzll(q), 64);
                }
#pragma unroll
                for (int m = 0; m < SG_LANE_MAX_K; ++m) in = in && g.lane != ch[m];
                const uint64_t key = (uint64_t)__double_as_longlong(d2);
                const bool take = in && (key < bk || (key == bk && i < bs));
                bk = take ? key : bk;
                bs = take ? i : bs;
            }
            wave_min(bk, bs);
            if (bk == KEY_NONE) break; // (the same in every lane: no candidate is left)
            const int q = __builtin_amdgcn_readfirstlane(L.seg[bs].lane);
#pragma unroll
            for (int m = 0; m < SG_LANE_MAX_K; ++m) ch[m] = m == j ? q : ch[m];
            if (lane == j) mine = bs;
            ++found;
        }
    }
    if (lane == 0 && count) count[o] = total;
    const int groups = n_ahead + 1, W = 6 + 2 * n_ahead;
    for (int t0 = 0; t0 < k * groups; t0 += 64) { // (uniform trip count: the cross-lane read is the whole wavefront's)
        const int item = t0 + lane, j = min(item / groups, SG_LANE_MAX_K - 1), m = item - (item / groups) * groups;
        const int best = __shfl(mine, j, 64);
        if (item >= k * groups) continue;
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int q = -1;
        if (j < found) {
            const LaneSeg g = L.seg[best];
            q = g.lane;
            const SegmentView sv = segment_view(g, f.x, f.y, f.s, f.c);
            if (m == 0) {
                v[0] = sv.offset; v[1] = sv.cos_err; v[2] = sv.sin_err;
                v[3] = sv.arc; v[4] = L.lane[q].total - sv.arc; v[5] = __builtin_sqrt(sv.d2);
            } else {
                double x, y;
                lane_point_ahead(L, q, sv.arc + (double)m * spacing, x, y);
                f.to_frame(x - f.x, y - f.y, v[0], v[1]);
            }
        }
        double *row = feat + ((size_t)o * k + j) * W;
        if (m == 0) {
#pragma unroll
            for (int c = 0; c < 6; ++c) row[c] = v[c];
            if (lanes) lanes[(size_t)o * k + j] = q < 0 ? -1 : q - L.net[net].lane0;
        } else {
            row[4 + 2 * m] = v[0];
            row[5 + 2 * m] = v[1];
        }
    }
}
#endif // SG_UNIT_OBS

// ------------------------------------------------------------------------------------------------
// The range scan: a fan of beams from an observer's pose point, each reporting the distance to the first other entity's box
// it meets and how fast that distance changes (no counterpart in the reference, whose RasterizedMapSensor is the image-shaped
// equivalent).  The definition is in include/sgym.h at sg_range_scan: a slab test of the beam in the entity's frame, plain
// unfused fp64 with IEEE divisions.  (SG_SCAN_MAX_RAYS: include/sgym.h.)
// ------------------------------------------------------------------------------------------------

// what a beam needs of one entity, computed once per observer: the observer's position in the entity's frame, the box slabs
// there, cos / sin of the entity's heading, its velocity relative to the observer's
struct ScanRow {
    double ox, oy, xlo, xhi, ylo, yhi, ce, se, dvx, dvy;
};

// one slab of the definition: the parameters at which o + t * l enters and leaves [lo, hi] (a beam along the slab is inside
// for every t or for none)
__device__ __forceinline__ void scan_slab(double o, double l, double lo, double hi, double &tn, double &tf)
{
    const double t1 = (lo - o) / l, t2 = (hi - o) / l;
    const bool along = l == 0.0, inside = o >= lo && o <= hi, up = t1 < t2;
    tn = along ? (inside ? -__builtin_inf() : __builtin_inf()) : (up ? t1 : t2);
    tf = along ? (inside ? __builtin_inf() : -__builtin_inf()) : (up ? t2 : t1);
}

// Observer o < n: observer_of; feat [n][n_rays][2] (range, range rate), slots [n][n_rays] (may be nullptr), hits [n]
// (may be nullptr), every byte written.  One wavefront per observer, four observers per workgroup, no barrier.  The scenario's
// slots go by in blocks of 64, ascending, through the wavefront's own LDS rows:
//   phase one, lane = entity: presence, sin / cos of its heading, the ScanRow -- once per observer and block of beams, not once
//     per beam -- and whether any beam can reach the box at all: a hit needs both slabs entered by max_range, and with
//     |l| <= 1 + a few ulp a slab whose two bounds lie on one side of the origin, both more than g away, is entered no sooner
//     than g * (1 - 1e-15) or lies behind the beam; so g > max_range * (1 + 1e-9) on either axis rules the entity out, with
//     the very subtractions the slab test divides (bounds in either order: extents may be negative).  A NaN keeps the entity in.
//   phase two, lane = beam: the rows of the entities within reach, a wavefront-uniform bit mask walked upwards, read as LDS
//     broadcasts; (best, slot, rate) with a strict <, so ascending slots give the tie rule with no cross-lane step.
// More than 64 beams go block by block of 64, each with phase one anew (some hundred instructions beside 64 slab tests per row).
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void range_scan_kernel(Params p, const int32_t *obs_scen, const int32_t *obs_slot, int64_t n, int n_rays,
                                                                double angle0, double dangle, double max_range, double *feat, int32_t *slots,
                                                                int32_t *hits)
{
    __shared__ ScanRow rows[4][64];
    int lane; int64_t o;
    if (!wave_item(n, lane, o)) return; // (the whole wavefront, which meets no barrier)
    const int w = wave_index();
    const Observer f = observer_of(p, obs_scen, obs_slot, o);
    const double reach = max_range * 1.000000001;
    int total = f.present ? 0 : -1;
    for (int b0 = 0; b0 < n_rays; b0 += 64) {
        const int b = b0 + lane;
        double best = __builtin_inf(), rate = 0.0;
        int slot = -1;
        if (f.present) {
            double sb, cb;
            sg_sincos(angle0 + (double)b * dangle, sb, cb);
            const double ux = cb * f.c - sb * f.s, uy = sb * f.c + cb * f.s;
            for (int e0 = 0; e0 < p.E; e0 += 64) {
                const ObservedSlot es = observed_slot(p, f, e0 + lane);
                const double *d = es.dyn, *st = es.stat;
                ScanRow q;
                sg_sincos(d[(SG_F_POSE + 3) * 64], q.se, q.ce);
                const double dx = f.x - d[(SG_F_POSE + 0) * 64], dy = f.y - d[(SG_F_POSE + 1) * 64];
                const double W = st[ST_BW * 64], L = st[ST_BL * 64], cx = st[ST_BCX * 64], cy = st[ST_BCY * 64];
                q.ox = dx * q.ce + dy * q.se;
                q.oy = dy * q.ce - dx * q.se;
                q.xlo = cx - 0.5 * L; q.xhi = cx + 0.5 * L;
                q.ylo = cy - 0.5 * W; q.yhi = cy + 0.5 * W;
                q.dvx = d[(SG_F_VEL + 0) * 64] - f.vx;
                q.dvy = d[(SG_F_VEL + 1) * 64] - f.vy;
                const double x1 = q.xlo - q.ox, x2 = q.xhi - q.ox, y1 = q.ylo - q.oy, y2 = q.yhi - q.oy;
                const bool out_of_reach = (x1 > reach && x2 > reach) || (x1 < -reach && x2 < -reach) || (y1 > reach && y2 > reach) ||
                                          (y1 < -reach && y2 < -reach);
                const bool present = es.present();
                tile_sync<1>(); // (the previous block's rows have been read)
                rows[w][lane] = q;
                tile_sync<1>();
                for (uint64_t todo = __ballot(es.other && present && !out_of_reach); todo; todo &= todo - 1) {
                    const int j = __builtin_ctzll(todo);
                    const ScanRow g = rows[w][j];
                    const double lx = ux * g.ce + uy * g.se, ly = uy * g.ce - ux * g.se;
                    double tnx, tfx, tny, tfy;
                    scan_slab(g.ox, lx, g.xlo, g.xhi, tnx, tfx);
                    scan_slab(g.oy, ly, g.ylo, g.yhi, tny, tfy);
                    double tmin = 0.0;
                    if (tnx > tmin) tmin = tnx;
                    if (tny > tmin) tmin = tny;
                    const double tmax = tfy < tfx ? tfy : tfx;
                    const bool take = tmin <= tmax && tmin <= max_range && tmin < __builtin_inf() && tmin < best;
                    best = take ? tmin : best;
                    slot = take ? e0 + j : slot;
                    rate = take ? g.dvx * ux + g.dvy * uy : rate;
                }
            }
            total += __popcll(__ballot(b < n_rays && slot >= 0));
        }
        if (b < n_rays) {
            double *row = feat + ((size_t)o * n_rays + b) * 2; // (16 bytes per lane, consecutive lanes consecutive beams)
            row[0] = !f.present ? 0.0 : slot >= 0 ? best : max_range;
            row[1] = rate;
            if (slots) slots[(size_t)o * n_rays + b] = slot;
        }
    }
    if (lane == 0 && hits) hits[o] = total;
}
#endif // SG_UNIT_OBS

// ------------------------------------------------------------------------------------------------
// The entity status: what a per-agent reward and termination ask of one entity -- in the scene, in a collision and with what,
// on the road, its speed and distance travelled, and the clearance, the distance from its box to the nearest other box (the
// reference asks ego_collision / ego_off_road of entities[0] alone, state/state.py:397-408).  The definition is in
// include/sgym.h at sg_entity_status: plain unfused fp64 with IEEE division and square root.
// ------------------------------------------------------------------------------------------------

// the smallest finite squared distance from the four corners of P to the four edges i -> (i + 1) & 3 of Q, folded into `best`
// (+inf to begin with: a NaN or an infinite d2 is never taken); the point-to-segment rule of lane_project
__device__ __forceinline__ double status_corners_to_edges(const double (&P)[8], const double (&Q)[8], double best)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        const double ax = Q[2 * i], ay = Q[2 * i + 1], bx = Q[2 * j], by = Q[2 * j + 1];
        const double ex = bx - ax, ey = by - ay, L2 = ex * ex + ey * ey;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double px = P[2 * k], py = P[2 * k + 1];
            const double wx = px - ax, wy = py - ay, t = (wx * ex + wy * ey) / L2;
            const bool at_a = L2 == 0.0 || !(t > 0.0), at_b = t >= 1.0;
            const double cx = at_a ? ax : at_b ? bx : ax + t * ex, cy = at_a ? ay : at_b ? by : ay + t * ey;
            const double dx = px - cx, dy = py - cy, d2 = dx * dx + dy * dy;
            best = d2 < best ? d2 : best;
        }
    }
    return best;
}

// Observer o < n: observer_of; flags [n], info [n][SG_ST_NINFO] (may be nullptr), feat [n][SG_ST_NFEAT] (may be nullptr),
// every byte written.  One wavefront per observer, four observers per workgroup, no LDS, no barrier, no atomics.  Its corners
// and its collision row's word of the block at hand belong to the observer alone, like its pose: every lane has them for itself.
//   the row: lane l takes the words l, l + 64, ... (one word up to 64 slots, at most 256): set bits, the lowest, and the entity
//     type of every set slot; a butterfly sums, takes the minimum and ORs.
//   the clearance: the scenario's slots go by in blocks of 64, ascending, lane = entity.  A lane whose bit of the row is set
//     has gap2 = +0.0; the other present ones get sin / cos of their heading, their corners, and the 32 corner-to-edge tests;
//     a block in which no lane has such a test to run (nobody present, or everybody in the row) skips them.  Per lane a running
//     (gap2 bits, slot) with a strict <, then wave_min: a finite non-negative double orders as its bit pattern does.
//     No pre-filter: every candidate is tested, so the answers are those of the plain definition by construction.
//   the surfaces: lane 0 looks up the pose point for all eight layers, lanes 1..4 a corner each for the driveable surface.
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void entity_status_kernel(Params p, const int32_t *obs_scen, const int32_t *obs_slot, int64_t n,
                                                                   uint32_t *flags, int32_t *info, double *feat)
{
    int lane; int64_t o;
    if (!wave_item(n, lane, o)) return; // (the whole wavefront, which meets no barrier)
    const Observer f = observer_of(p, obs_scen, obs_slot, o);
    if (!f.present) { // not in State.poses: the rule for an absent entities[0]
        if (lane == 0) flags[o] = SG_ST_OFF_ROAD;
        if (info && lane < SG_ST_NINFO) info[(size_t)o * SG_ST_NINFO + lane] = -1;
        if (feat && lane < SG_ST_NFEAT) feat[(size_t)o * SG_ST_NFEAT + lane] = 0.0;
        return;
    }
    const ObservedSlot own = observed_slot(p, f, f.slot);
    const double *d = own.dyn, *st = own.stat;
    double A[8];
    sg_corners(f.x, f.y, f.s, f.c, st[ST_BW * 64], st[ST_BL * 64], st[ST_BCX * 64], st[ST_BCY * 64], A);

    // the collision row
    const uint64_t *row = reinterpret_cast<const uint64_t *>(d) + SG_F_COLL * 64; // word q: row[q * 64]
    const int W = p.FROWS - SG_F_COLL;                                             // (64 * W >= E)
    int pop = 0, low = INDEX_NONE;
    uint32_t hit = 0u;
    for (int q = lane; q < W; q += 64) {
        uint64_t m = row[(size_t)q * 64];
        pop += __popcll(m);
        if (m && low == INDEX_NONE) low = q * 64 + __builtin_ctzll(m); // (ascending q: this lane's lowest)
        for (; m; m &= m - 1) {
            const int e = q * 64 + __builtin_ctzll(m);
            if (e >= p.E) continue; // (a row holds entity slots only)
            const int64_t meta = reinterpret_cast<const int64_t *>(entity_stat(p, (uint32_t)f.r * p.EP + (uint32_t)e))[ST_META * 64];
            const int etype = (int)((meta >> 8) & 0xff);
            hit |= etype == 0 ? SG_ST_HIT_VEHICLE : etype == 1 ? SG_ST_HIT_PEDESTRIAN : SG_ST_HIT_OTHER;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        pop += __shfl_xor(pop, m, 64);
        low = min(low, __shfl_xor(low, m, 64));
        hit |= (uint32_t)__shfl_xor((int)hit, m, 64);
    }

    // the clearance
    uint64_t bk = KEY_NONE;
    int bs = INDEX_NONE;
    for (int e0 = 0; e0 < p.E; e0 += 64) {
        const int e = e0 + lane;
        const ObservedSlot es = observed_slot(p, f, e);
        const double *de = es.dyn, *se = es.stat;
        const bool in = es.other && es.present();
        const bool bit = ((row[(size_t)(e0 >> 6) * 64] >> lane) & 1ull) != 0;
        double g = __builtin_inf();
        if (sg_any(in && !bit)) {
            double B[8], sb, cb;
            sg_sincos(de[(SG_F_POSE + 3) * 64], sb, cb);
            sg_corners(de[(SG_F_POSE + 0) * 64], de[(SG_F_POSE + 1) * 64], sb, cb, se[ST_BW * 64], se[ST_BL * 64], se[ST_BCX * 64],
                       se[ST_BCY * 64], B);
            g = status_corners_to_edges(A, B, g);
            g = status_corners_to_edges(B, A, g);
        }
        g = bit ? 0.0 : g;
        const uint64_t key = in && g < __builtin_inf() ? (uint64_t)__double_as_longlong(g) : KEY_NONE;
        const bool take = key < bk; // (ascending slots per lane: the lower slot keeps a tie)
        bk = take ? key : bk;
        bs = take ? e : bs;
    }
    wave_min(bk, bs);

    // the surfaces: the pose point (every layer) and the four corners (the driveable surface)
    uint32_t lay = 0u;
    if (lane < 5 && p.road) {
        const RoadIndex RI = *p.road;
        const double px = lane == 0 ? f.x : lane == 1 ? A[0] : lane == 2 ? A[2] : lane == 3 ? A[4] : A[6];
        const double py = lane == 0 ? f.y : lane == 1 ? A[1] : lane == 2 ? A[3] : lane == 3 ? A[5] : A[7];
        lay = rn_layers_at(RI, RI.net_of_scen[f.r], lane == 0 ? 0xffu : SG_LAYER_DRIVEABLE, px, py);
    }
    const int corners_on = __popcll(__ballot(lane >= 1 && lane < 5 && (lay & SG_LAYER_DRIVEABLE) != 0));
    const uint32_t lay0 = (uint32_t)__shfl((int)lay, 0, 64);

    if (lane == 0)
        flags[o] = SG_ST_PRESENT | (pop ? SG_ST_COLLISION : 0u) | ((lay0 & SG_LAYER_DRIVEABLE) ? 0u : SG_ST_OFF_ROAD) |
                   (corners_on < 4 ? SG_ST_CORNER_OFF : 0u) | hit | (lay0 << SG_ST_LAYER_SHIFT);
    if (info && lane < SG_ST_NINFO)
        info[(size_t)o * SG_ST_NINFO + lane] = lane == 0 ? pop : lane == 1 ? (low == INDEX_NONE ? -1 : low) : lane == 2 ? corners_on
                                                                                                              : (bk == KEY_NONE ? -1 : bs);
    if (feat && lane < SG_ST_NFEAT) {
        const double speed = sg_norm3(d[(SG_F_VEL + 0) * 64], d[(SG_F_VEL + 1) * 64], d[(SG_F_VEL + 2) * 64]);
        const double gap = bk == KEY_NONE ? __builtin_inf() : __builtin_sqrt(__longlong_as_double((long long)bk));
        feat[(size_t)o * SG_ST_NFEAT + lane] = lane == 0 ? speed : lane == 1 ? d[SG_F_DIST * 64] : gap;
    }
}
#endif // SG_UNIT_OBS

// ------------------------------------------------------------------------------------------------
// The route and recorded-track observation: where an observer is relative to the route it was given (sg_set_routes) and to
// where its own recording has it at the scenario's time -- progress along the route, what is left of it, points ahead, and the
// displacement from the log (no counterpart in the reference, whose entities replay or are driven, never compared).  The
// definition is in include/sgym.h at sg_route_observation: plain unfused fp64 with IEEE division and square root.  The route
// rows are LaneSeg rows built by sg_set_routes exactly as sg_set_lanes builds its own, read through polyline_nearest,
// segment_view and polyline_point_at (sgym_polyline.hpp); the recorded pose is own_position_clamped; presence and the entity
// frame are Observer's.
// ------------------------------------------------------------------------------------------------
struct RouteIndex {      // device pointers, by value; route_of == nullptr: no routes set
    const int32_t *route_of; // [R * EP] padded entity index -> route, -1 where the entity has none
    const int32_t *seg_off;  // [n_routes + 1] ranges of seg
    const double *total;     // [n_routes] cum + len of the route's last segment (0 without segments)
    const LaneSeg *seg;      // the segments of every route, route by route
};

// Observer o < n: observer_of; feat [n][SG_RT_NFEAT + 2 * n_ahead], info [n][SG_RT_NINFO] (may be nullptr), every byte
// written.  One wavefront per observer, four per workgroup, no LDS, no barrier, no atomics.  Its recorded pose and the best row
// belong to the observer alone, like its pose: every lane computes them for itself.
//   phase one, lane = route segment: polyline_nearest.  Every lane then projects onto the best row again (segment_view): the
//     same operations on the same operands, so the same bits.
//   phase two, lane m - 1 = look-ahead point m: its own polyline_point_at.
//   the store, lane = feature: the row is at most 11 + 2 * 16 = 43 doubles, one pass; the look-ahead pairs come from their lanes
//     by a cross-lane read.
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void route_observation_kernel(Params p, RouteIndex P, const int32_t *obs_scen, const int32_t *obs_slot,
                                                                       int64_t n, int n_ahead, double spacing, double *feat, int32_t *info)
{
    int lane; int64_t o;
    if (!wave_item(n, lane, o)) return; // (the whole wavefront, which meets no barrier)
    const int W = SG_RT_NFEAT + 2 * n_ahead;
    const Observer f = observer_of(p, obs_scen, obs_slot, o);
    double *row = feat + (size_t)o * W;
    if (!f.present) { // not in State.poses
        if (lane < W) row[lane] = 0.0;
        if (info && lane < SG_RT_NINFO) info[(size_t)o * SG_RT_NINFO + lane] = -1;
        return;
    }
    const uint32_t idx = (uint32_t)f.r * p.EP + (uint32_t)f.slot;

    // the recorded track
    const int64_t *sti = reinterpret_cast<const int64_t *>(entity_stat(p, idx));
    const int n_k = (int)(sti[ST_META * 64] >> 32);
    double tr0 = 0.0, tr1 = 0.0, tr2 = 0.0, tr3 = 0.0, tr4 = 0.0;
    int when = 2;
    if (n_k > 0) {
        const double *kn = p.knots + sti[ST_KNOT_OFF * 64] * 7;
        const double t = p.sdyn[f.r].t;
        double rec[6], sr, cr;
        own_position_clamped(kn, n_k, t, rec);
        const double X = rec[0] - f.x, Y = rec[1] - f.y;
        sg_sincos(rec[3], sr, cr);
        f.to_frame(X, Y, tr0, tr1);
        tr2 = __builtin_sqrt(X * X + Y * Y);
        f.to_frame(cr, sr, tr3, tr4);
        when = t < kn[0] ? -1 : t > kn[(size_t)(n_k - 1) * 7] ? 1 : 0;
    }

    // the route: phase one
    const int route = P.route_of ? P.route_of[idx] : -1;
    const int s0i = route >= 0 ? P.seg_off[route] : 0, s1i = route >= 0 ? P.seg_off[route + 1] : 0;
    const int best = polyline_nearest(P.seg, s0i, s1i, lane, f.x, f.y); // (the same in every lane)
    SegmentView sv = {0.0, 0.0, 0.0, 0.0, 0.0};
    double left = 0.0, dist = 0.0, ah0 = 0.0, ah1 = 0.0;
    if (best >= 0) {
        sv = segment_view(P.seg[s0i + best], f.x, f.y, f.s, f.c);
        const double total = P.total[route];
        left = total - sv.arc;
        dist = __builtin_sqrt(sv.d2);
        // phase two
        if (lane < n_ahead) {
            double x, y;
            polyline_point_at(P.seg, s0i, s1i, total, sv.arc + (double)(lane + 1) * spacing, x, y);
            f.to_frame(x - f.x, y - f.y, ah0, ah1);
        }
    }

    // the store (the cross-lane reads are the whole wavefront's)
    const int from = lane >= SG_RT_NFEAT ? (lane - SG_RT_NFEAT) >> 1 : 0; // (< 64)
    const double a0 = __shfl(ah0, from, 64), a1 = __shfl(ah1, from, 64);
    if (lane < W) {
        const double v = lane == 0 ? tr0 : lane == 1 ? tr1 : lane == 2 ? tr2 : lane == 3 ? tr3 : lane == 4 ? tr4
                       : lane == 5 ? sv.offset : lane == 6 ? sv.cos_err : lane == 7 ? sv.sin_err : lane == 8 ? sv.arc
                       : lane == 9 ? left : lane == 10 ? dist : ((lane - SG_RT_NFEAT) & 1) ? a1 : a0;
        row[lane] = v;
    }
    if (info && lane < SG_RT_NINFO) info[(size_t)o * SG_RT_NINFO + lane] = lane == 0 ? best : when;
}
#endif // SG_UNIT_OBS

// ------------------------------------------------------------------------------------------------
// The time to collision: when an observer's box will touch another one if both keep their velocity and heading, for how long,
// and which face meets first (no counterpart in the reference, whose FutureCollisionDetector replays recordings and answers
// with one bit).  The definition is in include/sgym.h at sg_time_to_collision: two rectangles are disjoint iff one of their four
// face normals separates them, so the contact interval is the intersection of four slab intervals; plain unfused fp64 with
// IEEE division.
// ------------------------------------------------------------------------------------------------

// one slab of the definition: the times at which the offset o + t * l enters and leaves [-H, H] (an offset that does not change
// is inside for every t or for none)
__device__ __forceinline__ void ttc_slab(double o, double l, double H, double &tn, double &tf)
{
    const double t1 = (-H - o) / l, t2 = (H - o) / l;
    const bool still = l == 0.0, inside = __builtin_fabs(o) <= H, up = t1 < t2;
    tn = still ? (inside ? -__builtin_inf() : __builtin_inf()) : (up ? t1 : t2);
    tf = still ? (inside ? __builtin_inf() : -__builtin_inf()) : (up ? t2 : t1);
}

// Observer o < n: observer_of; feat [n][SG_TTC_NFEAT], info [n][SG_TTC_NINFO] (may be nullptr), every byte written.  One
// wavefront per observer, four observers per workgroup, no LDS, no barrier, no atomics.  Its box, like its pose, belongs to the
// observer alone: every lane has it for itself.  The scenario's slots go by in blocks of 64, ascending, lane = entity: presence,
// the bit of the observer's collision row, sin / cos of the entity's heading, the four slabs; a block in which no lane has a
// candidate skips them.  Per lane a running (tmin bits, slot) with a strict < and beside it what the outputs need of that pair;
// wave_min makes the key the wavefront's, and the rest comes from the lane that owns the winning slot by a cross-lane read (it is
// that lane's own best: the lowest of its slots with the smallest key).  The count is a ballot per block.
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void time_to_collision_kernel(Params p, const int32_t *obs_scen, const int32_t *obs_slot, int64_t n,
                                                                       double horizon, double *feat, int32_t *info)
{
    int lane; int64_t o;
    if (!wave_item(n, lane, o)) return; // (the whole wavefront, which meets no barrier)
    const Observer f = observer_of(p, obs_scen, obs_slot, o);
    if (!f.present) { // not in State.poses
        if (lane < SG_TTC_NFEAT) feat[(size_t)o * SG_TTC_NFEAT + lane] = 0.0;
        if (info && lane < SG_TTC_NINFO) info[(size_t)o * SG_TTC_NINFO + lane] = -1;
        return;
    }
    const ObservedSlot own = observed_slot(p, f, f.slot);
    const double Wo = own.stat[ST_BW * 64], Lo = own.stat[ST_BL * 64], cxo = own.stat[ST_BCX * 64], cyo = own.stat[ST_BCY * 64];
    const double px = f.x + (cxo * f.c - cyo * f.s), py = f.y + (cxo * f.s + cyo * f.c);
    const uint64_t *row = reinterpret_cast<const uint64_t *>(own.dyn) + SG_F_COLL * 64; // word q: row[q * 64] (64 * words >= E)

    uint64_t bk = KEY_NONE;
    int bs = INDEX_NONE, b_axis = -1, total = 0;
    double b_until = 0.0, b_l0 = 0.0, b_l1 = 0.0;
    for (int e0 = 0; e0 < p.E; e0 += 64) {
        const int e = e0 + lane;
        const ObservedSlot es = observed_slot(p, f, e);
        const double *d = es.dyn, *st = es.stat;
        const bool in = es.other && es.present();
        if (!sg_any(in)) continue; // (the same in every lane)
        const bool bit = ((row[(size_t)(e0 >> 6) * 64] >> lane) & 1ull) != 0;
        double sn, cn;
        sg_sincos(d[(SG_F_POSE + 3) * 64], sn, cn);
        const double We = st[ST_BW * 64], Le = st[ST_BL * 64], cxe = st[ST_BCX * 64], cye = st[ST_BCY * 64];
        const double qx = d[(SG_F_POSE + 0) * 64] + (cxe * cn - cye * sn), qy = d[(SG_F_POSE + 1) * 64] + (cxe * sn + cye * cn);
        const double dx = qx - px, dy = qy - py, wx = d[(SG_F_VEL + 0) * 64] - f.vx, wy = d[(SG_F_VEL + 1) * 64] - f.vy;
        const double cr = cn * f.c + sn * f.s, sr = sn * f.c - cn * f.s;
        const double ao[4] = {dx * f.c + dy * f.s, dy * f.c - dx * f.s, dx * cn + dy * sn, dy * cn - dx * sn};
        const double al[4] = {wx * f.c + wy * f.s, wy * f.c - wx * f.s, wx * cn + wy * sn, wy * cn - wx * sn};
        const double aH[4] = {0.5 * Lo + 0.5 * (__builtin_fabs(Le * cr) + __builtin_fabs(We * sr)),
                              0.5 * Wo + 0.5 * (__builtin_fabs(Le * sr) + __builtin_fabs(We * cr)),
                              0.5 * Le + 0.5 * (__builtin_fabs(Lo * cr) + __builtin_fabs(Wo * sr)),
                              0.5 * We + 0.5 * (__builtin_fabs(Lo * sr) + __builtin_fabs(Wo * cr))};
        double tmin = 0.0, tmax = __builtin_inf();
        int axis = -1;
        bool nan = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) { // (registers: only ever indexed by this unrolled loop)
            double tn, tf;
            ttc_slab(ao[i], al[i], aH[i], tn, tf);
            nan = nan || ao[i] != ao[i] || al[i] != al[i] || aH[i] != aH[i];
            if (tn > tmin) { tmin = tn; axis = i; }
            if (tf < tmax) tmax = tf;
        }
        const bool meets = !nan && tmin <= tmax && tmin <= horizon && tmin < __builtin_inf();
        tmin = bit ? 0.0 : tmin;  // the state's own predicate decides the present
        axis = bit ? -1 : axis;
        const bool contact = in && (bit || meets);
        total += __popcll(__ballot(contact));
        const uint64_t key = contact ? (uint64_t)__double_as_longlong(tmin) : KEY_NONE;
        const bool take = key < bk; // (ascending slots per lane: the lower slot keeps a tie)
        bk = take ? key : bk;
        bs = take ? e : bs;
        b_until = take ? (tmax > tmin ? tmax : tmin) : b_until;
        b_l0 = take ? al[0] : b_l0;
        b_l1 = take ? al[1] : b_l1;
        b_axis = take ? axis : b_axis;
    }
    wave_min(bk, bs);
    const bool threat = bk != KEY_NONE;
    const int from = threat ? (bs & 63) : 0; // (the cross-lane reads are the whole wavefront's)
    const double until = __shfl(b_until, from, 64), l0 = __shfl(b_l0, from, 64), l1 = __shfl(b_l1, from, 64);
    const int axis = __shfl(b_axis, from, 64);
    if (lane < SG_TTC_NFEAT) {
        const double v = lane == 0 ? __longlong_as_double((long long)bk) : lane == 1 ? until : lane == 2 ? l0 : l1;
        feat[(size_t)o * SG_TTC_NFEAT + lane] = threat ? v : lane == 0 ? __builtin_inf() : 0.0;
    }
    if (info && lane < SG_TTC_NINFO) info[(size_t)o * SG_TTC_NINFO + lane] = lane == 1 ? total : !threat ? -1 : lane == 0 ? bs : axis;
}
#endif // SG_UNIT_OBS

// ------------------------------------------------------------------------------------------------
// The surface scan: a fan of beams from an observer's pose point, each reporting per requested road layer the range at which
// it first changes side of that layer's surface (no counterpart in the reference; range_scan_kernel is the half that sees
// boxes).  The definition is in include/sgym.h at sg_surface_scan: a coarse march of n_steps samples `step` apart over the
// exact point predicate rn_layers_at (sgym_road.hpp), then n_refine bisections of the step that flipped; plain unfused fp64.
// ------------------------------------------------------------------------------------------------
struct SurfLayers {
    uint32_t bit[8]; // one SG_LAYER_* bit per requested layer, 0 behind the last (by value: no device copy)
};

// Observer o < n: observer_of; feat [n][n_layers][n_rays], flags [n][n_layers][n_rays] (may be nullptr), hits [n][n_layers]
// (may be nullptr), every byte written.  One wavefront per observer, four observers per workgroup, no LDS, no barrier, no
// atomics; nothing of the other entities is read, so the scenario's width does not matter.  The beams go by in blocks of 64:
//   the march, lane = beam: one rn_layers_at per sample with want = the layers of the list that have not flipped yet on this
//     beam -- one cell lookup answers all of them, and a layer's answer does not depend on what else is asked for --, the step
//     of the first flip per list entry in registers (indexed by unrolled loops only); the wavefront leaves the march once no
//     live lane has a layer left.  The hit counts are ballots, the same in every lane.
//   the bisections, lane = (beam, list entry): pair q of the block is beam q % nb, entry q / nb (nb: the block's beams), in
//     rounds of 64 pairs.  A bisection is n_refine dependent lookups, so with few beams and several layers (16 x 3) one round
//     does what a lane = beam loop over the layers would do in three, and with 64 beams and one layer the two are the same.  A
//     pair's lane fetches the beam's direction and first-flip step from the beam's lane (cross-lane reads by the whole
//     wavefront) and writes the pair's outputs itself: consecutive lanes, consecutive beams of one layer.
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void surface_scan_kernel(Params p, const int32_t *obs_scen, const int32_t *obs_slot, int64_t n,
                                                                  SurfLayers lay, int n_layers, int n_rays, double angle0, double dangle,
                                                                  double step, int n_steps, int n_refine, double *feat,
                                                                  unsigned char *flags, int32_t *hits)
{
    int lane; int64_t o;
    if (!wave_item(n, lane, o)) return; // (the whole wavefront, which meets no barrier)
    const Observer f = observer_of(p, obs_scen, obs_slot, o);
    const size_t row0 = (size_t)o * n_layers;
    if (!f.present) { // not in State.poses
        for (size_t i = lane; i < (size_t)n_layers * n_rays; i += 64) {
            feat[row0 * n_rays + i] = 0.0;
            if (flags) flags[row0 * n_rays + i] = 0;
        }
        if (hits && lane < n_layers) hits[row0 + lane] = -1;
        return;
    }
    uint32_t want = 0u;
#pragma unroll
    for (int l = 0; l < 8; ++l) want |= lay.bit[l];
    RoadIndex RI{};
    int net = -1;
    if (p.road) {
        RI = *p.road;
        net = RI.net_of_scen[f.r];
    }
    const uint32_t s0 = rn_layers_at(RI, net, want, f.x, f.y); // (the pose point itself: the same in every lane)
    const double reach = (double)n_steps * step;
    int count[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // (the same in every lane)

    for (int b0 = 0; b0 < n_rays; b0 += 64) {
        const int b = b0 + lane;
        double sb, cb;
        sg_sincos(angle0 + (double)b * dangle, sb, cb);
        const double ux = cb * f.c - sb * f.s, uy = sb * f.c + cb * f.s;

        // the march
        int first[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t pending = (b < n_rays && net >= 0) ? want : 0u;
        for (int k = 1; k <= n_steps && sg_any(pending != 0u); ++k) {
            const double t = (double)k * step;
            uint32_t flip = 0u;
            if (pending) flip = (rn_layers_at(RI, net, pending, f.x + t * ux, f.y + t * uy) ^ s0) & pending;
#pragma unroll
            for (int l = 0; l < 8; ++l) first[l] = (flip & lay.bit[l]) ? k : first[l];
            pending &= ~flip;
        }
#pragma unroll
        for (int l = 0; l < 8; ++l) count[l] += __popcll(__ballot(first[l] > 0));

        // the bisections
        const int nb = min(64, n_rays - b0), pairs = nb * n_layers;
        for (int q0 = 0; q0 < pairs; q0 += 64) {
            const int q = q0 + lane;
            const bool valid = q < pairs;
            const int l = valid ? q / nb : 0, from = valid ? q - l * nb : 0;
            const double bux = __shfl(ux, from, 64), buy = __shfl(uy, from, 64);
            int k = 0;
            uint32_t bit = 0u;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int km = __shfl(first[m], from, 64);
                k = m == l ? km : k;
                bit = m == l ? lay.bit[m] : bit;
            }
            const uint32_t side0 = s0 & bit;
            const bool hit = valid && k > 0;
            double hi = reach;
            if (hit) {
                double lo = (double)(k - 1) * step;
                hi = (double)k * step;
                for (int i = 0; i < n_refine; ++i) {
                    const double mid = (lo + hi) * 0.5;
                    const bool across = rn_layers_at(RI, net, bit, f.x + mid * bux, f.y + mid * buy) != side0;
                    hi = across ? mid : hi;
                    lo = across ? lo : mid;
                }
            }
            if (valid) {
                const size_t at = (row0 + l) * n_rays + b0 + from; // (consecutive lanes, consecutive beams of one layer)
                feat[at] = hi;
                if (flags) flags[at] = (unsigned char)((hit ? 1u : 0u) | (side0 ? 2u : 0u));
            }
        }
    }
    if (hits && lane < n_layers) {
        int c = 0;
#pragma unroll
        for (int l = 0; l < 8; ++l) c = lane == l ? count[l] : c;
        hits[row0 + lane] = c;
    }
}
#endif // SG_UNIT_OBS

// ------------------------------------------------------------------------------------------------
// The pose history: where an observer and the k entities nearest to it were at the last n_samples record rows, `stride` rows
// apart, in the observer's CURRENT frame (no counterpart in the reference, whose State.recorded_poses hands the whole record to
// the host).  The definition is in include/sgym.h at sg_pose_history: the neighbours are those of nearest_kernel at the current
// state (near_neighbours), the rows come from the pose record the stepping kernels append to (p.rec_pose, p.rec_t; row
// rec_rows - 1 is the current state), plain unfused fp64 as near_store computes its rows.  (SG_HIST_MAX_SAMPLES,
// SG_HIST_MAX_STRIDE: include/sgym.h.)
// ------------------------------------------------------------------------------------------------
#ifdef SG_UNIT_OBS // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
// the subject slots of the wide path: neighbour i of the workgroup's observer at [i - 1]
__device__ __forceinline__ int *hist_subjects()
{
    __shared__ int subject[SG_NEAR_MAX_K];
    return subject;
}

// Observer o < n: observer_of.  feat [n][1 + k][n_samples][6] fp64, slots [n][k] (may be nullptr), count [n] (may be nullptr),
// every byte written.  0 <= k <= 32, 1 <= n_samples <= 64, stride >= 1.  Subject 0 is the observer, subject i >= 1 neighbour
// i - 1 of near_neighbours.  count: the candidates within the radius; -2 for a stale record (rec_rows != n_steps + 1: the record
// filled up and the scenario went on stepping), else -1 for an observer that is not present; both with slots -1 and zero rows.
// NB > 0 (scenarios of at most NB * 64 <= 512 entities): one wavefront per observer, four observers per workgroup, no LDS, no
// barrier.  After the selection lane i - 1 holds neighbour i; the (subject, sample) pairs go by 64 at a time, pair q = sample
// q / (1 + k) of subject q % (1 + k) -- subject fastest: for one row and coordinate the slots of a scenario lie within EP * 8
// bytes, so the 64 loads of a plane touch the few cache lines of 64 / (1 + k) rows -- and a lane fetches its subject's slot from
// the lane that holds it (a cross-lane read by the whole wavefront).  Per pair three 8-byte loads (the x, y and heading planes
// of the row), the row's time, one sg_sincos, six stores.  Row offsets are 64-bit: rec_cap * 6 * R * EP exceeds 2^31.
// NB == 0 (the wide path): one workgroup per observer; wavefront 0's neighbours go through LDS and all 256 threads walk the pairs.
template <int NB>
static __global__ __launch_bounds__(256) void pose_history_kernel(Params p, const int32_t *obs_scen, const int32_t *obs_slot, int64_t n,
                                                                  int n_samples, int stride, int k, double r2, double *feat, int32_t *slots,
                                                                  int32_t *count)
{
    int lane; int64_t o;
    if (!wave_item(n, lane, o, NB == 0)) return; // (NB > 0: the whole wavefront, which meets no barrier)
    const int w = wave_index();
    const Observer f = observer_of(p, obs_scen, obs_slot, o);
    const sg_scenario_state &sd = p.sdyn[f.r];
    const double t = sd.t;
    const int L = sd.rec_rows;
    const int status = L != sd.n_steps + 1 ? -2 : f.present ? 0 : -1; // (the same in every lane; on the wide path in the whole workgroup)
    int nb = -1, total = status;
    if (status == 0) nb = near_neighbours<NB>(p, f, max(k, 1), r2, lane, w, total); // (k == 0: the count alone)
    if (NB || w == 0) {
        if (lane == 0 && count) count[o] = total;
        if (lane < k && slots) slots[(size_t)o * k + lane] = nb;
    }
    if constexpr (NB == 0) {
        if (w == 0 && lane < SG_NEAR_MAX_K) hist_subjects()[lane] = nb;
        __syncthreads();
    }
    const int S = 1 + k, pairs = S * n_samples;
    const int step = NB ? 64 : 256, me = NB ? lane : (int)threadIdx.x;
    const size_t plane = (size_t)p.R * p.EP;
    const double *rec = p.rec_pose + (size_t)f.r * p.EP;
    double *out = feat + (size_t)o * pairs * 6;
    for (int q0 = 0; q0 < pairs; q0 += step) { // (uniform trip count: the cross-lane read is the whole wavefront's)
        const int q = q0 + me, j = q / S, i = q - j * S;
        int e;
        if constexpr (NB > 0) e = __shfl(nb, max(i - 1, 0), 64);
        else e = hist_subjects()[max(i - 1, 0)];
        e = i == 0 ? f.slot : e;
        if (q >= pairs) continue;
        const int rho = L - 1 - j * stride; // (j * stride < 2^26)
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (status == 0 && e >= 0 && rho >= 0 && rho < p.rec_cap) {
            const double *row = rec + (size_t)rho * 6 * plane + e;
            const double X = row[0], Y = row[plane], Hd = row[3 * plane], tr = p.rec_t[(size_t)rho * p.R + f.r];
            if (X == X) { // (an absent entity's row is NaN in all six coordinates)
                double se, ce;
                sg_sincos(Hd, se, ce);
                f.to_frame(X - f.x, Y - f.y, v[0], v[1]);
                f.to_frame(ce, se, v[2], v[3]);
                v[4] = j == 0 ? 0.0 : t - tr;
                v[5] = 1.0;
            }
        }
        double *dst = out + ((size_t)i * n_samples + j) * 6; // (48 bytes per lane)
#pragma unroll
        for (int m = 0; m < 6; ++m) dst[m] = v[m];
    }
}
#endif // SG_UNIT_OBS

} // namespace sg
