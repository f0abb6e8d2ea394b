// sgym_host.hpp -- what the host units of libsgym_hip.so share (private: the public side is include/sgym.h).
// The handle, the error and allocation helpers, and the declarations of the few internal functions that cross unit
// boundaries (namespace sgh).  The units: sgym_hip.hip (the dispatcher and the stepping entry points), h_handle.hip, h_upload.hip,
// h_queue.hip, h_slice.hip, h_wide.hip, h_rss.hip, h_road.hip, h_observe.hip, h_drive.hip, h_episode.hip, h_snapshot.hip, h_read.hip, h_group.hip.  None of them holds a
// kernel: they launch through sgym_launch.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <atomic>
#include <cassert>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <iterator>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "sgym_launch.hpp"

using sg::Params;

namespace sgh {

// Device allocations of one upload, kept across uploads: a pipeline that feeds batch after batch of the same shape through
// a handle must not pay hipFree / hipMalloc each time (both wait for the WHOLE device, i.e. for the rollout another handle
// is running: the double-buffered upload of tools/upload_time.py would serialise with it).  sg_upload requests its buffers
// in a fixed order; request i reuses slot i when it is large enough.
struct ReusePool {
    std::vector<void *> ptr;
    std::vector<size_t> cap;
    size_t cursor = 0;
    void rewind() { cursor = 0; }
};

// One buffer of the handle that grows on demand: device memory, device memory that is poisoned when fresh (SG_POISON), or
// page-locked host memory.  ensure() frees, allocates and poisons, nothing else: whatever a site does around a growth
// (waiting for the stream before the old buffer goes, ++generation after) stays with the site.
struct GrowBuf {
    enum Kind { DEVICE, DEVICE_POISONED, HOST };
    explicit GrowBuf(Kind k) : kind(k) {}
    void *ptr = nullptr;
    size_t cap = 0; // bytes
    const Kind kind;
    int ensure(sg_handle *h, size_t bytes, bool *grew = nullptr); // room for `bytes`; *grew: the buffer is a new one
    void release();
    template <typename T> T *as() const { return static_cast<T *>(ptr); }
};

// A list of (scenario, slot) pairs on the device (sg_set_observers, sg_set_drivers): [2][capacity] int32_t, the scenarios in the
// first half of the buffer, the slots in the second (grown on demand).  n: the pairs set (0: none); sg_upload forgets them.
struct EntityList {
    GrowBuf buf{GrowBuf::DEVICE};
    int64_t n = 0;
    int32_t *scenarios() const { return buf.as<int32_t>(); }
    int32_t *slots() const { return buf.as<int32_t>() + buf.cap / (2 * sizeof(int32_t)); }
    // replaces the list by n > 0 checked pairs (check_pairs): waits for the stream (something queued may still read the previous
    // list); from there on the old list is gone: a failure of the runtime leaves an empty one (h_observe.hip)
    int upload(sg_handle *h, int64_t n_new, const int32_t *scenario, const int32_t *slot);
    void release() { buf.release(); }
};

} // namespace sgh

// The fields are grouped by the unit that owns them, in the order of the units.
struct sg_handle {
    // ---- h_handle.hip: the shape (sg_create), the streams, the tuning, the error text ----
    sg_config cfg{};
    int R = 0, E = 0, EP = 0, G = 0, WV = 1;
    size_t NE = 0; // padded entity count
    bool wide = false;                           // more than 512 entities per scenario: the multi-kernel step (sgym_wide.hpp)
    hipStream_t stream = nullptr;
    hipStream_t ctl_stream = nullptr; // the controller pre-pass (sg::control_kernel) and the knot copy of sg_upload
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int n_simd = 1024;                                       // SIMDs of the device (4 per compute unit)
    int tab_min = 16, chunk_steps = 1024, overlap = 1; // sg_set_tuning
    int slice_mode = 1;       // sg_set_tuning / env SG_SLICE: 0 never, 1 automatic (small batches, long rollouts)
    bool quiet = true;              // env SG_QUIET=0: every step of the table rollout kernels runs the whole collision pass (Params::quiet)
    int queue_mode = 1;             // env SG_QUEUE=0: the chunk launches of rounds 1-4 instead
    int ctl_slice = 64;                                // steps per control_kernel launch (env SG_CTL_SLICE)
    int ped_serial = 0;                                // env SG_PED_SERIAL: pedestrian pair loop one pedestrian per lane
    int crowd_kernel = 1;     // env SG_CROWD_KERNEL=0: all-pedestrian batches take the general pedestrian variant too
    bool crowd_models = true, models_all_sf = true; // env SG_CROWD_MODELS; every model of sg_set_ped_models is a SocialForce
    double c_tol = 0.4;                                // CollisionMetric(c_tol): angular half-width of a box corner, metrics/collision.py:57
    uint64_t generation = 0, tick_gen = ~0ull;         // bumped by every call that changes what the kernels are launched with
    std::string err;

    // ---- h_upload.hip: the batch (sg_upload), its pedestrian settings, the resets ----
    bool uploaded = false;
    bool has_ped = false;
    bool planar = false;      // every knot of the batch has z = pitch = roll = +0.0 (bit patterns): rollout_kernel_tab_planar
    bool sliceable = false;   // every entity is a replay entity / replay agent / PID or vehicle agent (or padding): the batch
                              // can be time-sliced (launch_sliced)
    bool all_ped = false;     // every entity of the batch is a pedestrian agent of catalog type Pedestrian (or padding)
    bool crowd_riders = false; // a crowd (64-lane tiles) whose other lanes are replay entities / replay agents / PID / vehicle agents:
                               // rollout_kernel_crowd_riders + control_kernel_riders (env SG_CROWD_RIDERS=0: the general variant)
    bool ego_first = true;                                 // every scenario's ego is its entity 0
    Params p{};
    sgh::ReusePool static_allocs, state_allocs;
    int32_t *d_row_scen = nullptr;
    int64_t total_rows = 0;
    std::vector<hipEvent_t> up_ev;  // sg_upload: one event per piece of the knot copy
    std::vector<double> up_grid_t;  // host buffers of sg_upload, kept between calls
    sgh::GrowBuf up_stat{sgh::GrowBuf::HOST}; // (page-locked)
    std::vector<int32_t> up_row_scen;
    std::vector<std::vector<double>> up_grids;
    // controller pre-pass (sg::control_kernel): controlled lanes of the batch
    int n_ctl = 0;
    int n_ext = 0;            // SG_KIND_AGENT_EXTERNAL slots in the batch
    double *d_ext = nullptr;  // [NE][6]
    int max_ctl_per_block = 0; // controlled lanes in the fullest 64-slot block
    std::vector<double> clock_t0;  // distinct scenario start times (ScenarioGym.get_start_time): one clock each
    std::vector<int> clock_of;     // [R]
    std::vector<uint8_t> slot_empty;                   // [R * E] the slot is SG_KIND_NONE in the uploaded batch (what sg_set_observers refuses)
    unsigned char *d_reset_mask = nullptr;             // [R] sg_reset_scenarios
    sg_social_force sf{};
    int ped_behaviour = 0;        // sg_set_ped_behaviour
    int n_ped_models = 0;         // sg_set_ped_models: > 1 = the batch mixes behaviour models / parameter sets
    double *d_ped_models = nullptr;  // [n_ped_models][PM_W]
    int32_t *d_model_of = nullptr;   // [NE]
    int noise_mode = 0;           // sg_set_ped_noise
    double noise_std[2] = {0.0, 0.0};
    double *d_normals = nullptr;  // [R][noise_len]
    long long noise_len = 0;
    unsigned long long noise_seed = 0;
    double *d_gon = nullptr;

    // ---- sgym_hip.hip: the dispatcher and the stepping entry points ----
    sgh::GrowBuf actions{sgh::GrowBuf::DEVICE};   // the actions of sg_step / sg_tick ([n][R][2] doubles)
    char last_kernel[96] = {0};     // sg_last_kernel
    bool timed = false;
    std::vector<hipEvent_t> ev_pool;
    int n_launches = 0;           // rollout_kernel launches of the last call
    std::vector<int> launch_ev;   // their (start, stop) event indices into ev_pool

    // ---- h_queue.hip: the table path as one persistent launch (sgym_queue.hpp, launch_queue), and as chunk launches ----
    sgh::GrowBuf qwords{sgh::GrowBuf::DEVICE}; // queue state + progress words, unsigned: [Q_PROG_STRIDE] the state words on a line of their own, [n_ctl_waves * Q_PROG_STRIDE] one
                                               // pre-pass progress word per 128-byte line, [nblk] block progress, [Q_MAX_CHUNKS + 1] chunk counters, [Q_SEATS] (+ [nblk] trace)
    double *d_qtab = nullptr;       // the table ring
    size_t qtab_bytes = 0;
    int q_waves_per_cu[3] = {-1, -1, -1}; // occupancy of rollout_kernel_tabq / _planar / _rss_tabq (slots_of), queried once per G
    int q_waves_G = 0;                    // ... the tile width they were queried for
    // page-locked copies of the queue state words (give-up code, items done) of the persistent launches that have not been looked
    // at yet (check_queue): a ring with one slot per launch, so that a second launch before the check cannot overwrite the
    // first one's code.  A give-up is STICKY: every later call that runs or reads the batch fails with its message until
    // sg_reset / sg_upload start the batch anew (the state is undefined in between).
    unsigned *q_host = nullptr;
    int q_head = 0, q_count = 0;    // next slot to use; launches not yet looked at
    bool q_failed = false;
    char q_msg[320] = {0};
    int last_schedule = 0;          // 0: not the table path, 1: chunk launches, 2: the persistent queue launch
    int last_chunks = 0, last_ring = 0, last_grid = 0;
    double *d_tab[4] = {nullptr, nullptr, nullptr, nullptr}; // controller-table buffers (launch_table: two, four with block groups)
    int n_tab = 0;
    size_t tab_bytes = 0;     // bytes of each table buffer

    // ---- h_slice.hip: the time-sliced rollout ----
    std::vector<void *> slice_allocs; // device arrays of launch_sliced, kept between calls of the same shape
    int slice_T = -1, slice_S = 0;
    sg::SliceArgs slice_args{};
    int *d_n_final = nullptr, *d_slice_done = nullptr;
    double *d_slice_tab = nullptr; // the controller table of a whole sliced call (batches with PID / vehicle agents)
    double *d_clock_t0 = nullptr;

    // ---- h_wide.hip ----
    std::vector<void *> wide_allocs;
    sg::WideArgs wide_args{};
    int *wide_running = nullptr;    // page-locked ring of "scenarios still running" answers (launch_wide)
    unsigned wide_check = 0;        // check points enqueued so far

    // ---- h_rss.hip ----
    int32_t *d_rss_state = nullptr, *d_rss_code = nullptr; // [NE] sg_rss_update
    int32_t *d_rss_seen = nullptr;                         // [R]
    bool rss_enabled = false;                              // sg_set_rss: RSSDistances runs after every step of sg_rollout / sg_step
    double *d_rss_safe = nullptr;                          // [NE][2]
    double *d_rssq = nullptr;                              // line-test queues of rollout_kernel_rss: [NE / 64][(rssq_steps + 1) * 64][12]
    int32_t *d_rssq_n = nullptr;                           // [NE / 64]
    int rssq_steps = 0;                                    // steps per launch the queues are sized for
    size_t rss_NE = 0, rssq_NE = 0;                        // padded entity counts the records / the queues were allocated for
    bool rss_stale = true;                                 // the records belong to a batch that is gone (sg_upload): cleared on next use

    // ---- h_observe.hip: the tick and the observations ----
    // sg_tick: the kernels of one RL tick captured once as a hipGraph and replayed with a single launch
    hipGraphExec_t tick_exec = nullptr;
    double tick_w = 0, tick_h = 0;
    int tick_nw = 0, tick_nh = 0, tick_nl = 0;
    bool tick_rss = false;                             // the captured step runs the RSS callback (rollout_kernel_rss* + rss_lines_kernel)
    int32_t tick_layers[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    sgh::GrowBuf term_flags{sgh::GrowBuf::DEVICE};     // [R] uint32_t, sg_terminal_flags
    sgh::GrowBuf obs{sgh::GrowBuf::DEVICE_POISONED};   // device scratch of the observation calls (grown on demand)

    // ---- h_road.hip ----
    std::vector<void *> road_allocs;                   // sg_set_road_networks
    sg::RoadIndex road{};                              // host copy of the device pointers (raster kernels take it by value)
    bool has_road = false;
    sg::RoadGeom geom{};                               // ... and of the per-geometry lists beside it (sg_road_info; arrays in road_allocs)
    sgh::GrowBuf road_info{sgh::GrowBuf::DEVICE_POISONED}; // device scratch of sg_road_info / sg_road_info_points (grown on demand)
    std::vector<void *> lane_allocs;                   // sg_set_lanes
    sg::LaneIndex lanes{};                             // host copy of its device pointers (seg == nullptr: no lanes set); sg_upload and
                                                       // sg_set_road_networks forget them (forget_lanes)

    // ---- h_observe.hip: the observers ----
    sgh::EntityList observers;                         // sg_set_observers
    sgh::GrowBuf routes{sgh::GrowBuf::DEVICE};         // sg_set_routes: the route totals, the segment rows, the segment ranges and the
                                                       // entity -> route map, one behind the other (grown on demand)
    sg::RouteIndex route{};                            // ... its pointers into that buffer (route_of == nullptr: no routes); sg_upload
                                                       // forgets them (forget_routes)

    // ---- h_drive.hip: the drivers ----
    std::vector<uint8_t> slot_external;                // [R * E] the slot is SG_KIND_AGENT_EXTERNAL in the uploaded batch (what sg_set_drivers asks for)
    sgh::EntityList drivers;                           // sg_set_drivers
    sgh::GrowBuf drv_actions{sgh::GrowBuf::DEVICE};    // host actions of drivers_step ([n_steps][drivers.n][2] doubles): not `actions`, whose
                                                       // address the captured tick graph holds
    sgh::GrowBuf policy{sgh::GrowBuf::DEVICE};         // sg_set_driver_policy: the parameter rows, the path totals, the segment rows, the policy
                                                       // list and the segment ranges, one behind the other (grown on demand)
    sg::PolicyIndex pol{};                             // ... its pointers into that buffer (driver == nullptr: no policy)
    int64_t n_pol = 0;                                 // policy drivers set (0: none); sg_set_drivers and sg_upload forget them
    sgh::GrowBuf pol_actions{sgh::GrowBuf::DEVICE};    // drivers_step with the policy: the caller's actions with the policy's rows merged in
                                                       // ([n_steps][drivers.n][2] doubles; a caller's device buffer is never written)
    sgh::GrowBuf pol_out{sgh::GrowBuf::DEVICE_POISONED}; // device scratch of sg_driver_policy_actions with host outputs

    // ---- h_episode.hip: the multi-agent tick (sg_tick_drivers) ----
    sgh::GrowBuf episode{sgh::GrowBuf::DEVICE};        // the accounting (prev_s, return, length, prev_ok: one behind the other at the front, so
                                                       // that one memset starts it anew) and every array of sg_episode_view
    size_t ep_state_bytes = 0;                         // ... the bytes of that front part
    int64_t ep_n = -1;                                 // the number of drivers the buffer is laid out for (-1: not laid out)
    bool ep_live = false;                              // the accounting holds episodes in progress; false (sg_reset, sg_upload, sg_set_drivers,
                                                       // sg_set_routes): the next tick zeroes it first
    sg::EpisodeArgs ep{};                              // the kernel's pointers into the buffer
    sg_episode_view ep_view{};                         // ... and the caller's

    // ---- h_read.hip ----
    // page-locked staging of sg_read_metrics (the per-scenario state and the event table travel every time metrics are read:
    // 0.5 + up to 6 MB for 4096 scenarios; pageable copies ran at a third of the PCIe rate)
    sgh::GrowBuf pin_sd{sgh::GrowBuf::HOST}, pin_ev{sgh::GrowBuf::HOST};

    // ---- h_snapshot.hip: the snapshots (sg_snapshot_create) ----
    std::vector<sg_snapshot *> snapshots;              // the ones alive (sg_destroy frees them)
    uint64_t upload_gen = 0, drivers_gen = 0;          // bumped by sg_upload / sg_set_drivers: a snapshot made before is of no use after
    int snap_d2d = 0;                                  // env SG_SNAP_D2D=1: a NULL-mask save / restore as one device-to-device copy per array
};

namespace sgh {

// the RSSDistances records hold results of the current batch (sg_upload leaves the buffers, not their contents)
inline bool rss_live(const sg_handle *h) { return h->d_rss_state && !h->rss_stale; }

// the crowd variants (rollout_kernel_crowd / _riders / _models) hold the social force model alone
// (several models: a pass of the force code per model, as the general variant does it -- up to four, SocialForce all of them)
inline bool crowd_allowed(const sg_handle *h)
{
    return h->crowd_kernel && h->ped_behaviour == SG_PED_SOCIAL_FORCE && (h->n_ped_models <= 1 || (h->n_ped_models <= 4 && h->models_all_sf && h->crowd_models));
}

inline int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}
// ... and a road network only as the source of the boundary forces (social_force.py:86-104: a phase behind the neighbour sums,
// gated on the launch having polygons at all); ego_off_road needs the cell lookup of rollout_kernel_road / the general variants
inline bool crowd_road_ok(const sg_handle *h) { return !h->has_road || (!(h->cfg.terminal_mask & SG_TERM_EGO_OFF_ROAD) && env_int("SG_CROWD_ROADS", 1) != 0); }

// Host threads for sg_upload's pass over the scenarios: the logical CPUs, capped at 64 and by the cgroup CPU quota (a box can
// show 256 CPUs under a quota of 16: more busy threads than that are throttled, not run -- ADVICE r2); SG_UPLOAD_THREADS overrides.
inline unsigned host_threads()
{
    static const unsigned n = [] {
        unsigned v = std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) { // cgroup v2: "<quota> <period>" or "max <period>"
            char q[32] = {0};
            long period = 0;
            if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
                const long quota = atol(q);
                if (quota > 0) v = std::min<unsigned>(v, (unsigned)std::max(1L, (quota + period - 1) / period));
            }
            fclose(f);
        }
        const int forced = env_int("SG_UPLOAD_THREADS", 0);
        return forced > 0 ? (unsigned)forced : v;
    }();
    return n;
}

// the message of a failed call: on the handle, or (h == nullptr: sg_create, sg_group_create) per thread (h_handle.hip)
extern thread_local std::string g_create_err;
int fail(sg_handle *h, int code, const char *fmt, ...);

#define HIP_TRY(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return sgh::fail(h, SG_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                             __FILE__, __LINE__);                                                 \
    } while (0)

// SG_POISON=1 (tests): every device array that is handed out WITHOUT being zeroed is filled with 0xA5 bytes instead of being
// left as the allocator found it -- a read of something no kernel wrote shows in a fresh process as it would after a
// thousand other handles (tests/test_gpu_parity.py::test_poisoned_allocations_change_nothing).  Synchronous, so that a fill can never land after a copy another stream makes into the same array.
inline int poison_byte() // 0: off; else the byte (SG_POISON=165: 0xA5, 255: NaNs / -1, 127: huge ints, NaN-free doubles)
{
    static const int v = env_int("SG_POISON", 0) & 0xff;
    return v;
}
inline bool poison_allocs() { return poison_byte() != 0; }
inline void poison(hipStream_t s, void *ptr, size_t bytes) // (a fresh allocation no kernel has written yet)
{
    if (poison_allocs() && ptr) {
        (void)hipMemsetAsync(ptr, poison_byte(), bytes, s);
        (void)hipStreamSynchronize(s);
    }
}

// ---- the pool allocators: a list that is freed as a whole (std::vector<void *>), or slots that are reused (ReusePool) ----
template <typename T>
int dev_alloc(sg_handle *h, std::vector<void *> &pool, T **out, size_t n, bool zero = true)
{
    void *ptr = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HIP_TRY(h, hipMalloc(&ptr, bytes));
    pool.push_back(ptr);
    if (zero) HIP_TRY(h, hipMemsetAsync(ptr, 0, bytes, h->stream));
    else if (poison_allocs()) { // (synchronous: the array may be filled on another stream next, e.g. the knot copy of sg_upload)
        HIP_TRY(h, hipMemsetAsync(ptr, poison_byte(), bytes, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    *out = (T *)ptr;
    return SG_OK;
}

template <typename T>
int dev_alloc(sg_handle *h, ReusePool &pool, T **out, size_t n, bool zero = true)
{
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    const size_t i = pool.cursor++;
    if (i == pool.ptr.size()) { pool.ptr.push_back(nullptr); pool.cap.push_back(0); }
    if (pool.cap[i] < bytes) {
        if (pool.ptr[i]) HIP_TRY(h, hipFree(pool.ptr[i]));
        pool.ptr[i] = nullptr;
        pool.cap[i] = 0;
        HIP_TRY(h, hipMalloc(&pool.ptr[i], bytes));
        pool.cap[i] = bytes;
    }
    if (zero) HIP_TRY(h, hipMemsetAsync(pool.ptr[i], 0, bytes, h->stream));
    else if (poison_allocs()) {
        HIP_TRY(h, hipMemsetAsync(pool.ptr[i], poison_byte(), bytes, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    *out = (T *)pool.ptr[i];
    return SG_OK;
}

template <typename Pool, typename T>
int dev_upload(sg_handle *h, Pool &pool, const T **out, const std::vector<T> &v)
{
    T *d = nullptr;
    int rc = dev_alloc(h, pool, &d, v.size(), false);
    if (rc) return rc;
    if (!v.empty()) HIP_TRY(h, hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    *out = d;
    return SG_OK;
}

inline void free_pool(ReusePool &pool)
{
    for (void *ptr : pool.ptr)
        if (ptr) (void)hipFree(ptr);
    pool.ptr.clear();
    pool.cap.clear();
    pool.cursor = 0;
}

inline void free_pool(std::vector<void *> &pool)
{
    for (void *ptr : pool) (void)hipFree(ptr);
    pool.clear();
}

// the lanes of sg_set_lanes go with the networks they belong to (sg_set_road_networks, sg_upload, sg_destroy)
inline void forget_lanes(sg_handle *h)
{
    free_pool(h->lane_allocs);
    h->lanes = sg::LaneIndex{};
}

// the policy of sg_set_driver_policy goes with the driver list it indexes (sg_set_drivers, sg_upload); the buffer stays for the next one
inline void forget_driver_policy(sg_handle *h)
{
    h->n_pol = 0;
    h->pol = sg::PolicyIndex{};
}

// the routes of sg_set_routes belong to entities of a batch (sg_upload); the buffer stays for the next ones
inline void forget_routes(sg_handle *h) { h->route = sg::RouteIndex{}; }

// the episode accounting of sg_tick_drivers starts anew with the next tick (sg_reset, sg_upload, sg_set_drivers, sg_set_routes)
inline void forget_episodes(sg_handle *h) { h->ep_live = false; }

// The device rows of one polyline pts[i0 .. i1) ([..][2] doubles), appended to segs: one row per segment a -> b in point order -- a,
// e = b - a, L2 = ex*ex + ey*ey, len = sqrt(L2), cum = the sequential sum of the preceding len, b -- tagged (lane, first).  Returns
// the polyline's total, cum + len of its last segment (0 without segments).  What sg_set_lanes, sg_set_driver_policy and
// sg_set_routes build their rows with; the host units are compiled with -ffp-contract=off: the products and sums are the unfused
// ones the definitions in include/sgym.h name.
inline double append_segments(std::vector<sg::LaneSeg> &segs, const double *pts, int64_t i0, int64_t i1, int32_t lane, int32_t first)
{
    double cum = 0.0;
    bool any = false;
    for (int64_t i = i0; i + 1 < i1; ++i) {
        const double *a = pts + 2 * i, *b = a + 2;
        sg::LaneSeg g{};
        g.ax = a[0]; g.ay = a[1]; g.bx = b[0]; g.by = b[1];
        g.ex = g.bx - g.ax; g.ey = g.by - g.ay;
        g.L2 = g.ex * g.ex + g.ey * g.ey;
        g.len = std::sqrt(g.L2);
        g.cum = cum;
        g.lane = lane; g.first = first;
        cum = cum + g.len;
        segs.push_back(g);
        any = true;
    }
    return any ? segs.back().cum + segs.back().len : 0.0;
}

// The path table of sg_set_driver_policy and sg_set_routes on the host, and its upload (h_observe.hip).  The caller fills dbl and
// ints with its own leading entries; build() puts the total of every path behind the doubles, seg_off [m + 1] behind the ints and the
// rows of append_segments into segs, path by path.
struct PathTable {
    std::vector<double> dbl;
    std::vector<sg::LaneSeg> segs;
    std::vector<int32_t> ints;
    void build(int64_t m, const int64_t *pt_off, const double *pts); // (pt_off monotone from 0: the caller has checked it)
    // [doubles][LaneSeg rows][ints] into buf, behind a wait for the stream (something queued may still read the previous table; the
    // caller has forgotten its pointers: a failure of the runtime leaves the handle without a table); the three parts' addresses
    int upload(sg_handle *h, GrowBuf &buf, const double **d_dbl, const sg::LaneSeg **d_seg, const int32_t **d_ints) const;
};

// one group holding every block: an ordinary launch of a table variant
inline sg::TabGroups one_group(const sg_handle *h, const double *tab, int n_steps)
{
    sg::TabGroups tg{};
    tg.active = 1;
    tg.gsz = (int)std::max<size_t>(1, h->NE / 64);
    tg.n[0] = n_steps;
    tg.buf[0] = tab;
    tg.start0 = 0; tg.len0 = (unsigned)tg.gsz; tg.start1 = 0; tg.len1 = 0;
    return tg;
}

// grid of a launch of the one-wavefront-per-tile table kernels: the blocks of the active groups
inline dim3 tab_grid(const sg_handle *h, const sg::TabGroups &tg)
{
    return dim3((unsigned)std::min<size_t>(h->NE / 64, (size_t)tg.len0 + tg.len1));
}

// the rollout kernel families launch_variant launches (launchers: sgym_launch.hpp, one object per family)
enum class Fam { ROAD_W8, RSS_W8, PED_W8, PLAIN_W8, CROWD, CROWD_RIDERS, RSS_PED, RSS_ROAD, PED, RSS_TAB, RSS, ROAD, TAB, TAB_ROWS, PLAIN };

// What one call launches, decided by plan_call before anything is launched (the schedules: launch_plan)
enum Schedule { SCHED_WIDE, SCHED_STEPWISE, SCHED_ONE, SCHED_TAB_DUMMY, SCHED_TAB };
struct LaunchPlan {
    Schedule schedule = SCHED_ONE;
    Fam reset_fam = Fam::PLAIN; // the reset launch (the table path resets with the non-table variant)
    Fam fam = Fam::PLAIN;       // the step launches
    bool rss_lines = false;     // the kernel runs the RSS callback and fills the line-test queue: rss_lines_kernel after it
    bool rss_alone = false;     // rss_kernel after the reset and after every step
    bool off_road = false;      // ego_off_road_kernel after every step
    bool riders = false, rss_tab = false;
    int ctl = sgl::CTL_GENERAL, ctl_metrics = 1; // the controller pre-pass of the table path
    bool timed = false;         // the call records its timing events
};

// ---- sgym_hip.hip ----
LaunchPlan plan_call(const sg_handle *h, int n_steps, bool rss, bool allow_tab);
int launch_plan(sg_handle *h, const LaunchPlan &pl, int n_steps, int do_reset, int force, const double *d_actions);
int launch_rollout(sg_handle *h, int n_steps, int do_reset, int force, const double *d_actions, bool rss = false);
int launch_main(sg_handle *h, const LaunchPlan &pl, Fam fam, int n_steps, int do_reset, int force, const double *d_actions,
                const double *d_tab, size_t *ev_next, const sg::TabGroups *groups = nullptr);
int rss_fused_call(sg_handle *h, bool live_only, bool *fused, bool *fresh = nullptr);
int get_event(sg_handle *h, size_t idx, hipEvent_t *out);
int ensure_actions(sg_handle *h, size_t n, bool *grew = nullptr); // room for n doubles in h->actions
// n_steps forced steps of the whole batch with the per-scenario actions d_actions ([n_steps][R][2], DEVICE), enqueued, not waited
// for: what sg_step does between its argument handling and its wait (the RSS callback fused or as a call of its own per step)
int step_forced(sg_handle *h, int n_steps, const double *d_actions);
// sg_last_kernel of the schedules that launch from other units (every name the handle can report is written in sgym_hip.hip)
void note_wide(sg_handle *h);
void note_queue(sg_handle *h, bool rss);
void note_slice(sg_handle *h, bool tab);
// ---- h_upload.hip ----
// State.reset of the scenarios with d_mask[r] != 0 (DEVICE [R]), enqueued, not waited for: what sg_reset_scenarios does between its
// copy and its wait.  clear_episodes: their episode accounting starts anew too (sg_tick_drivers' own reset has done that already)
int reset_scenarios_queued(sg_handle *h, const uint8_t *d_mask, bool clear_episodes);
// ---- h_observe.hip ----
// What a list of n (scenario, slot) pairs requires of every pair beyond being in range (check_pairs): the slot holds an entity, it is an
// SG_KIND_AGENT_EXTERNAL slot, no pair is listed twice.
enum PairRules : unsigned { PAIR_HOLDS_ENTITY = 1u, PAIR_EXTERNAL = 2u, PAIR_ONCE = 4u };
int check_pairs(sg_handle *h, const char *who, int64_t n, const int32_t *scenario, const int32_t *slot, unsigned rules);
// ---- h_drive.hip ----
// n_steps steps of the batch, each with the drivers' controllers ahead of it and -- policy -- the policy ahead of them, enqueued, not
// waited for: what sg_step_drivers, sg_step_drivers_policy and sg_tick_drivers do between their checks and their end.  actions
// [n_steps][drivers.n][2]: HOST (copied; wait_host_copy: on the device when this returns, and that alone is waited for), DEVICE (read
// in place without the policy, never written) or null ((0, 0) for every driver)
int drivers_step(sg_handle *h, int n_steps, const double *actions, int32_t actions_device, bool policy, bool wait_host_copy);
// ---- h_episode.hip ----
// the episode buffer laid out for the current driver list (h->ep, h->ep_view, h->ep_state_bytes); a change of the number of drivers
// moves it and forgets the episodes
int episode_layout(sg_handle *h);
int episode_clear_masked(sg_handle *h, const uint8_t *d_mask); // (enqueued; nothing when no episode is in progress)
// ---- h_queue.hip ----
int check_queue(sg_handle *h);
void forget_queue_failure(sg_handle *h);
void drain_streams(sg_handle *h);
int launch_table(sg_handle *h, const LaunchPlan &pl, int n_steps, int force, const double *d_actions, size_t *ev_next);
// ---- h_slice.hip ----
// SG_OK, an error, or SG_SLICE_FALLBACK: the arrays could not be allocated -- the caller takes the step-by-step path
#define SG_SLICE_FALLBACK 1
bool slicing_pays(const sg_handle *h, int n_steps);
int launch_sliced(sg_handle *h, int n_steps);
// ---- h_wide.hip ----
int ensure_wide(sg_handle *h);
int launch_wide(sg_handle *h, int n_steps, int do_reset, int force, const double *d_actions, bool rss);
// ---- h_snapshot.hip ----
void free_snapshots(sg_handle *h); // (sg_destroy; the stream has been waited for)
// ---- h_rss.hip ----
int ensure_rss(sg_handle *h, bool *fresh);
int ensure_rssq(sg_handle *h);
void launch_rss_alone(sg_handle *h, int reset);

// ---- delivery of an observation (h_observe.hip, h_road.hip) ----
// the sticky give-up of check_queue for a call that does not wait for the stream: a launch still running is judged by the
// next call that synchronises
inline int queue_gave_up(sg_handle *h) { return h->q_failed ? fail(h, SG_ERR_HIP, "%s", h->q_msg) : SG_OK; }

// One output array of an observation call: the caller's pointer (null: an optional array that was not asked for) and its bytes.
struct OutPart {
    void *out;
    size_t bytes;
};

// Device scratch of the calls that deliver to the host, grown on demand behind a wait for the stream (something queued may still
// write the old one): a tick of an RL loop asks once per step, a hipMalloc / hipFree pair per call would cost more than the kernels.
// The observation scratch (h->obs) is the one whose address sg_tick's captured graph holds: its growth bumps the generation.  The
// others (h->pol_out, h->road_info) are apart from it because it holds what sg_raster_map_device / sg_tick handed out, which stays valid.
inline int scratch(sg_handle *h, GrowBuf &buf, size_t bytes, unsigned char **out)
{
    if (bytes > buf.cap) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (const int rc = buf.ensure(h, bytes)) return rc;
        if (&buf == &h->obs) ++h->generation;
    }
    *out = buf.as<unsigned char>();
    return SG_OK;
}

// Runs `launch(d)` -- hipError_t(void *const d[4]), the launches on the handle's stream -- with d[i] where part i is to be
// written, and delivers the parts (unused ones at the end: {}).  outputs_device: d[i] is the caller's pointer; stream-ordered, not waited for, what is
// known of the queue so far.  Else the parts lie one behind the other, in their order, from the start of the scratch `buf`
// (a part that was not asked for keeps its room and gets d[i] = null), with `tail` more bytes
// for the launch's own use behind them at the next multiple of 16, d[3]; one copy per part asked for, the wait for the stream,
// check_queue.  A failure of the HIP runtime reads "<who>: <step> failed: <error string>".
template <typename Launch>
int deliver(sg_handle *h, const char *who, bool outputs_device, GrowBuf &buf, const OutPart (&parts)[3], size_t tail, Launch launch)
{
    assert(tail == 0 || !outputs_device);
    const auto hip = [&](hipError_t e, const char *step) {
        return e == hipSuccess ? SG_OK : fail(h, SG_ERR_HIP, "%s: %s failed: %s", who, step, hipGetErrorString(e));
    };
    void *d[4] = {parts[0].out, parts[1].out, parts[2].out, nullptr};
    if (outputs_device) {
        if (const int rc = hip(launch(d), "the launch")) return rc;
        return queue_gave_up(h); // (not waited for: what is known so far)
    }
    const size_t bytes = parts[0].bytes + parts[1].bytes + parts[2].bytes, tail_off = (bytes + 15) & ~(size_t)15;
    unsigned char *base = nullptr;
    if (const int rc = scratch(h, buf, tail ? tail_off + tail : bytes, &base)) return rc;
    if (tail) d[3] = base + tail_off;
    for (int i = 0; i < 3; ++i) { if (parts[i].out) d[i] = base; base += parts[i].bytes; }
    if (const int rc = hip(launch(d), "the launch")) return rc;
    for (int i = 0; i < 3; ++i)
        if (parts[i].out && parts[i].bytes)
            if (const int rc = hip(hipMemcpyAsync(parts[i].out, d[i], parts[i].bytes, hipMemcpyDeviceToHost, h->stream), "hipMemcpyAsync")) return rc;
    if (const int rc = hip(hipStreamSynchronize(h->stream), "hipStreamSynchronize")) return rc;
    return check_queue(h); // (a persistent launch that gave up: sticky)
}

// What every observation of the egos or of the observers does behind its own argument checks: refuses a handle without a batch; n =
// the observers of sg_set_observers, or the ego of every scenario; n == 0: nothing is written; refuses a null primary output (part
// `primary` of `per`, named `primary_name`); then deliver() through the observation scratch with per[i].bytes PER OBSERVER, and
// launch(d, d_scen, d_slot, n) -- d_scen, d_slot: the observer list, null for the egos.
template <typename Launch>
int observe(sg_handle *h, const char *who, bool observers, bool outputs_device, int primary, const char *primary_name, const OutPart (&per)[3],
            Launch launch)
{
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    const int64_t n = observers ? h->observers.n : (int64_t)h->R;
    if (n == 0) return queue_gave_up(h); // no observers: nothing is written
    if (!per[primary].out) return fail(h, SG_ERR_INVALID, "%s: null %s", who, primary_name);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int32_t *d_scen = observers ? h->observers.scenarios() : nullptr, *d_slot = observers ? h->observers.slots() : nullptr;
    const OutPart all[3] = {{per[0].out, (size_t)n * per[0].bytes}, {per[1].out, (size_t)n * per[1].bytes}, {per[2].out, (size_t)n * per[2].bytes}};
    return deliver(h, who, outputs_device, h->obs, all, 0, [&](void *const *d) { return launch(d, d_scen, d_slot, n); });
}

} // namespace sgh
