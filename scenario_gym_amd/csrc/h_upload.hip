// h_upload.hip -- sg_upload: a batch of scenarios onto the device (the BatchReplayEntity union knot grids built on the host,
// sort/unique per scenario, threaded; everything else on the device), the resets and the pedestrian settings of a batch.
#include "sgym_host.hpp"

using namespace sgh;

extern "C" int sg_set_social_force(sg_handle *h, const sg_social_force *params)
{
    if (!h || !params) return SG_ERR_INVALID;
    h->sf = *params;
    h->p.sf = *params;
    ++h->generation;
    return SG_OK;
}

extern "C" int sg_set_ped_behaviour(sg_handle *h, int32_t behaviour)
{
    if (!h) return SG_ERR_INVALID;
    if (behaviour != SG_PED_SOCIAL_FORCE && behaviour != SG_PED_RANDOM_WALK)
        return fail(h, SG_ERR_INVALID, "sg_set_ped_behaviour: unknown behaviour %d", behaviour);
    if (h->uploaded && behaviour != h->ped_behaviour)
        return fail(h, SG_ERR_STATE, "sg_set_ped_behaviour: call before sg_upload (the batch's kernels are chosen there)");
    h->ped_behaviour = behaviour;
    h->p.ped_behaviour = behaviour;
    ++h->generation;
    return SG_OK;
}

static void apply_noise(sg_handle *h)
{
    h->p.noise_mode = h->noise_mode;
    h->p.noise_std_lon = h->noise_std[0];
    h->p.noise_std_lat = h->noise_std[1];
    h->p.noise_normals = h->d_normals;
    h->p.noise_len = h->noise_len;
    h->p.noise_seed = h->noise_seed;
}

// PedestrianAgent(..., behaviour=...) per agent (pedestrian/agent.py:18-41): the distinct models of the batch + the model of
// every entity slot.  One model: the handle-wide setters.
extern "C" int sg_set_ped_models(sg_handle *h, int32_t n_models, const sg_ped_model *models, const int32_t *model_of)
{
    if (!h) return SG_ERR_INVALID;
    if (n_models < 1 || n_models > SG_MAX_PED_MODELS || !models)
        return fail(h, SG_ERR_INVALID, "sg_set_ped_models: n_models=%d (1 .. %d) or null models", n_models, SG_MAX_PED_MODELS);
    if (h->uploaded) return fail(h, SG_ERR_STATE, "sg_set_ped_models: call before sg_upload (the batch's kernels are chosen there)");
    for (int m = 0; m < n_models; ++m) {
        if (models[m].behaviour != SG_PED_SOCIAL_FORCE && models[m].behaviour != SG_PED_RANDOM_WALK)
            return fail(h, SG_ERR_INVALID, "sg_set_ped_models: model %d: unknown behaviour %d", m, models[m].behaviour);
        if (!(models[m].std_lon >= 0.0) || !(models[m].std_lat >= 0.0))
            return fail(h, SG_ERR_INVALID, "sg_set_ped_models: model %d: std must be >= 0", m);
    }
    if (n_models > 1 && !model_of) return fail(h, SG_ERR_INVALID, "sg_set_ped_models: several models need model_of[n_scenarios * n_entities]");
    // (every refusal before anything of the handle changes: a refused call leaves the models it had)
    if (n_models > 1)
        for (int r = 0; r < h->R; ++r)
            for (int e = 0; e < h->E; ++e)
                if (model_of[(size_t)r * h->E + e] >= n_models)
                    return fail(h, SG_ERR_INVALID, "sg_set_ped_models: model_of[%d][%d] = %d >= n_models = %d", r, e, model_of[(size_t)r * h->E + e], n_models);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // model 0 is also what the handle-wide fields say (the single-model kernels, the oracle of a one-model batch)
    h->sf = models[0].params;
    h->p.sf = h->sf;
    h->ped_behaviour = models[0].behaviour;
    h->p.ped_behaviour = h->ped_behaviour;
    if (h->noise_mode != SG_NOISE_OFF) { h->noise_std[0] = models[0].std_lon; h->noise_std[1] = models[0].std_lat; }
    h->n_ped_models = n_models;
    h->models_all_sf = true;
    for (int m = 0; m < n_models; ++m) h->models_all_sf = h->models_all_sf && models[m].behaviour == SG_PED_SOCIAL_FORCE;
    if (n_models > 1) {
        std::vector<double> rows((size_t)n_models * sg::PM_W, 0.0);
        for (int m = 0; m < n_models; ++m) {
            double *r = rows.data() + (size_t)m * sg::PM_W;
            r[sg::PM_BEHAVIOUR] = (double)models[m].behaviour;
            memcpy(r + sg::PM_SF, &models[m].params, sizeof(sg_social_force));
            r[sg::PM_STD_LON] = models[m].std_lon; // (read only when the handle's noise mode is not off)
            r[sg::PM_STD_LAT] = models[m].std_lat;
        }
        std::vector<int32_t> mo(h->NE, 0);
        for (int r = 0; r < h->R; ++r)
            for (int e = 0; e < h->E; ++e) {
                const int32_t v = model_of[(size_t)r * h->E + e];
                mo[(size_t)r * h->EP + e] = v < 0 ? 0 : v;
            }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (h->d_ped_models) HIP_TRY(h, hipFree(h->d_ped_models));
        if (h->d_model_of) HIP_TRY(h, hipFree(h->d_model_of));
        h->d_ped_models = nullptr;
        h->d_model_of = nullptr;
        HIP_TRY(h, hipMalloc((void **)&h->d_ped_models, rows.size() * sizeof(double)));
        HIP_TRY(h, hipMalloc((void **)&h->d_model_of, mo.size() * sizeof(int32_t)));
        HIP_TRY(h, hipMemcpy(h->d_ped_models, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_model_of, mo.data(), mo.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    apply_noise(h);
    ++h->generation;
    return SG_OK;
}

extern "C" int sg_set_ped_noise(sg_handle *h, int32_t mode, double std_lon, double std_lat, const double *normals,
                                int64_t per_scenario, uint64_t seed)
{
    if (!h) return SG_ERR_INVALID;
    if (mode < SG_NOISE_OFF || mode > SG_NOISE_DEVICE) return fail(h, SG_ERR_INVALID, "sg_set_ped_noise: unknown mode %d", mode);
    if (!(std_lon >= 0.0) || !(std_lat >= 0.0)) return fail(h, SG_ERR_INVALID, "sg_set_ped_noise: std must be >= 0");
    if (mode == SG_NOISE_STREAM && (!normals || per_scenario < 2))
        return fail(h, SG_ERR_INVALID, "sg_set_ped_noise: SG_NOISE_STREAM needs [n_scenarios][per_scenario >= 2] variates");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->d_normals) { (void)hipFree(h->d_normals); h->d_normals = nullptr; }
    h->noise_len = 0;
    if (mode == SG_NOISE_STREAM) {
        const size_t n = (size_t)h->R * (size_t)per_scenario;
        HIP_TRY(h, hipMalloc((void **)&h->d_normals, n * sizeof(double)));
        HIP_TRY(h, hipMemcpy(h->d_normals, normals, n * sizeof(double), hipMemcpyHostToDevice));
        h->noise_len = per_scenario;
    }
    h->noise_mode = mode;
    h->noise_std[0] = mode == SG_NOISE_OFF ? 0.0 : std_lon;
    h->noise_std[1] = mode == SG_NOISE_OFF ? 0.0 : std_lat;
    h->noise_seed = seed;
    apply_noise(h);
    ++h->generation;
    return SG_OK;
}

// reference defaults: VehicleController.__init__ controller.py:64-70, PIDController.__init__ :154-161
// + PedestrianAgent / PedestrianController defaults, pedestrian/agent.py:18-27
static const double kDefaultCtrl[SG_NCTRL] = {0.7, 5.0, NAN, 0.0, 0.03054, 1.5709, 0.3753, 1.8970, 0.0204,
                                              0.0, 5.0, 0.0, 1.0, 0, 0, 0};

// ---- sg_upload, stage by stage ----------------------------------------------------------------------------------------
// the previous batch is forgotten: its buffers are reused, what belonged to it (networks, observers, RSS records) starts anew
static void forget_batch(sg_handle *h)
{
    h->static_allocs.rewind(); // (buffers of the previous batch are reused where they are large enough)
    h->state_allocs.rewind();
    free_pool(h->road_allocs); // the networks belong to a batch (net_of_scenario)
    forget_lanes(h);
    // the RSS records and the line-test queue (GiBs) belong to the handle's shape, not to the batch: they stay allocated and
    // start anew (ensure_rss / ensure_rssq on first use; a hipFree + hipMalloc of the queue per upload stalled every tenth
    // or so sg_upload of a sweep for a second)
    h->rss_stale = true;
    h->p.rss_state = nullptr; h->p.rss_code = nullptr; h->p.rss_seen = nullptr; h->p.rss_safe = nullptr;
    h->p.rssq = nullptr; h->p.rssq_n = nullptr;
    h->has_road = false;
    h->road = sg::RoadIndex{};
    h->geom = sg::RoadGeom{};
    h->observers.n = 0; // the observers are slots of a batch
    h->drivers.n = 0; // ... and so are the drivers
    forget_driver_policy(h); // ... whose list the policy indexes
    forget_routes(h);        // the routes belong to entities of a batch
    h->uploaded = false; // (the controller table buffers stay: launch_rollout regrows them when the new batch needs more)
    h->ego_first = true;
    ++h->generation;
    ++h->upload_gen; // (the snapshots of the previous batch can only be destroyed)
    free_pool(h->slice_allocs);
    h->slice_T = -1;
}

// what kind of batch this is -- which decides the tile width and the kernel families (pick_family)
static int classify_batch(sg_handle *h, const sg_scenarios *sc)
{
    // pedestrian agents are compiled for tiles of >= 16 lanes
    h->has_ped = false;
    h->all_ped = true;
    h->sliceable = true;
    h->slot_empty.resize((size_t)h->R * h->E);
    h->slot_external.resize((size_t)h->R * h->E);
    for (size_t i = 0; i < (size_t)h->R * h->E; ++i) {
        h->slot_empty[i] = sc->kind[i] == SG_KIND_NONE;
        h->slot_external[i] = sc->kind[i] == SG_KIND_AGENT_EXTERNAL;
        h->sliceable = h->sliceable && (sc->kind[i] == SG_KIND_NONE || sc->kind[i] == SG_KIND_REPLAY || sc->kind[i] == SG_KIND_AGENT_REPLAY ||
                                        sc->kind[i] == SG_KIND_AGENT_PID || sc->kind[i] == SG_KIND_AGENT_VEHICLE);
        h->has_ped = h->has_ped || sc->kind[i] == SG_KIND_AGENT_PEDESTRIAN;
        h->all_ped = h->all_ped && (sc->kind[i] == SG_KIND_NONE || (sc->kind[i] == SG_KIND_AGENT_PEDESTRIAN && sc->etype[i] == 1));
    }
    if (h->has_ped && h->WV == 1 && h->G < 16) { h->G = 16; h->EP = 16; h->NE = (((size_t)h->R * h->EP + 63) / 64) * 64; }
    h->crowd_riders = false;
    if (h->has_ped && !h->all_ped && h->G == 64 && h->WV <= 4 && crowd_allowed(h) && h->n_ped_models <= 1 /* (the riders variant knows one model) */ &&
        env_int("SG_CROWD_RIDERS", 1) != 0) {
        bool ok = true; // pedestrian agents of catalog type Pedestrian, and nothing the pre-pass cannot ride for
        for (size_t i = 0; i < (size_t)h->R * h->E && ok; ++i)
            ok = sc->kind[i] == SG_KIND_AGENT_PEDESTRIAN ? sc->etype[i] == 1 : sc->kind[i] != SG_KIND_AGENT_EXTERNAL;
        h->crowd_riders = ok;
    }
    if (h->has_ped && (!sc->route_off || !sc->routes)) return fail(h, SG_ERR_INVALID, "sg_upload: pedestrian agents need route_off/routes");
    // (257..512 entities: pedestrian agents run the general pedestrian variant, rollout_kernel<64, 8, true, false>; the crowd
    // kernels, the riders' pre-pass and road networks with pedestrians stop at 256)
    return SG_OK;
}

namespace {
// what one thread of the host pass brings back
struct UploadWorker {
    std::string err;
    int err_r = 0, ext_cnt = 0; // the scenario of `err` (R: none); SG_KIND_AGENT_EXTERNAL slots seen
    char ego_nz = 0;            // some ego is not entity 0
    std::vector<double> times, merged; // scratch of the union grid
};

// One sg_upload: what crosses its stages (nothing of it outlives the call).  The stages run in the order they are declared in.
struct Upload {
    sg_handle *const h;
    const sg_scenarios *const sc;
    const int R, E, EP; // (after classify_batch: pedestrian batches are promoted to tiles of 16 lanes)
    const size_t NE, nblk, stat_n;
    Params &p;
    std::vector<std::vector<double>> &grids; // BatchReplayEntity union knot grid per scenario (entity/batch.py:83-95)
    std::vector<double> &grid_t;
    std::vector<int32_t> &row_scen;
    // the knot copy
    static constexpr int UP_MAX = 4;
    int64_t rows_total = 0;
    double *d_knots = nullptr;
    int UP_CHUNKS = 1;
    int chunk_r[UP_MAX + 1];
    hipError_t copy_err = hipSuccess;
    std::atomic<int> issued{0};
    std::thread copier;
    // the host pass
    double *stat = nullptr;
    std::vector<int32_t> ctl_ent; // controlled lanes (PID / vehicle agents) in entity order
    std::vector<char> zpr_zero;   // [R] every knot of the scenario has z = pitch = roll = +0.0 (a planar recording: the usual case)
    int n_ext = 0;
    std::vector<sg::ScenStatic> sstat;
    std::vector<int64_t> grid_off;
    int64_t total_rows = 0;
    // SG_TRACE_UPLOAD: stage timings on stderr
    const bool trace;
    std::chrono::steady_clock::time_point t_last;

    Upload(sg_handle *h_, const sg_scenarios *sc_, std::chrono::steady_clock::time_point t_entry)
        : h(h_), sc(sc_), R(h_->R), E(h_->E), EP(h_->EP), NE(h_->NE), nblk(NE / 64), stat_n(nblk * sg::ST_COUNT * 64), p(h_->p),
          grids(h_->up_grids), grid_t(h_->up_grid_t), row_scen(h_->up_row_scen), trace(env_int("SG_TRACE_UPLOAD", 0) != 0), t_last(t_entry)
    {
    }
    ~Upload() { if (copier.joinable()) copier.join(); } // every return path waits for the copier

    void stage(const char *name)
    {
        if (!trace) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "sg_upload: %-28s %7.2f ms\n", name, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
    double &S(size_t ent, int f) const { return stat[(ent >> 6) * sg::ST_COUNT * 64 + (size_t)f * 64 + (ent & 63)]; }
    int64_t &SI(size_t ent, int f) const { return *reinterpret_cast<int64_t *>(&S(ent, f)); }
    void slot_defaults(size_t o) const // a padding slot: never present
    {
        for (int f = 0; f < sg::ST_COUNT; ++f) S(o, f) = 0.0;
        for (int q = 0; q < 4; ++q) S(o, sg::ST_BW + q) = 1.0;
        for (int q = 0; q < sg::NCTRL_ROWS; ++q) S(o, sg::ST_CTRL + q) = kDefaultCtrl[q];
        SI(o, sg::ST_META) = SG_KIND_NONE | (2 << 8);
        SI(o, sg::ST_CTL) = -1;
    }

    int start_knot_copy();
    int stat_buffer();
    bool scenario(int r, UploadWorker &w);
    int host_pass();
    void lay_out_grids();
    int static_arrays();
    int state_arrays();
    int resample();
};

int Upload::start_knot_copy()
{
    // ---- the knots (by far the largest array: 1.6 GB for 4096 x 64 x 128) start crossing PCIe NOW, from a thread of their
    // own on the second stream, while the host validates the batch and builds the union grids below.  Their extent comes
    // from knot_off, which is checked first (a bad offset must not turn into an out-of-bounds read of the copy).
    rows_total = sc->knot_off[(size_t)R * E];
    {
        bool ok = sc->knot_off[0] >= 0;
        for (size_t i = 0; i < (size_t)R * E && ok; ++i) ok = sc->knot_off[i + 1] >= sc->knot_off[i];
        if (!ok) return fail(h, SG_ERR_INVALID, "sg_upload: knot_off is not monotone");
    }
    {
        int rc0 = dev_alloc(h, h->static_allocs, &d_knots, (size_t)std::max<int64_t>(rows_total, 1) * 7, false);
        if (rc0) return rc0;
    }
    // The copy goes in UP_CHUNKS pieces on scenario boundaries, an event after each: the stage-1 resample of a piece's
    // scenarios (build_grid_kernel: resample) runs while the later pieces are still crossing.
    // Ordinary (pageable) host memory goes in one piece: the runtime stages it through its own buffers, and several large
    // copies in flight from such memory disturbed the host threads below (every other upload took 60 ms instead of 34).
    {
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, sc->knots) == hipSuccess && attr.type == hipMemoryTypeHost) UP_CHUNKS = UP_MAX;
        (void)hipGetLastError(); // (an unregistered pointer is reported as an error by some runtimes)
    }
    while (h->up_ev.size() < (size_t)UP_CHUNKS) {
        hipEvent_t e;
        HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->up_ev.push_back(e);
    }
    for (int c = 0; c <= UP_CHUNKS; ++c) chunk_r[c] = (int)((int64_t)R * c / UP_CHUNKS);
    copier = std::thread([&]() {
        if (rows_total > 0) copy_err = hipSetDevice(h->cfg.device);
        for (int c = 0; c < UP_CHUNKS && rows_total > 0 && copy_err == hipSuccess; ++c) {
            const int64_t a = sc->knot_off[(size_t)chunk_r[c] * E], b = sc->knot_off[(size_t)chunk_r[c + 1] * E];
            if (b > a)
                copy_err = hipMemcpyAsync(d_knots + a * 7, sc->knots + a * 7, (size_t)(b - a) * 7 * sizeof(double), hipMemcpyHostToDevice, h->ctl_stream);
            if (copy_err == hipSuccess) copy_err = hipEventRecord(h->up_ev[c], h->ctl_stream);
            issued.store(c + 1, std::memory_order_release);
        }
        issued.store(UP_CHUNKS, std::memory_order_release); // (also after an error: nobody waits for a piece that will not come)
        if (rows_total > 0 && copy_err == hipSuccess) copy_err = hipStreamSynchronize(h->ctl_stream);
    });
    return SG_OK;
}

// ---- validate + block re-layout + union knot grids (host, one parallel pass over the scenarios) ----
int Upload::stat_buffer()
{
    // (48 MB for 4096 x 64: every slot is written by the pass below.  This and the other host buffers of an upload belong to
    // the handle: mapping, faulting in and unmapping them anew took 6 ms of every call)
    // It is page-locked: the copy engine takes it from where the pass wrote it.
    if (const int rc = h->up_stat.ensure(h, stat_n * sizeof(double))) return rc;
    stat = h->up_stat.as<double>();
    for (size_t o = (size_t)R * EP; o < NE; ++o) slot_defaults(o); // the tail of the last block
    grids.resize(R);
    for (auto &g : grids) g.clear(); // (capacity stays)
    sstat.resize(R);
    return SG_OK;
}

// one scenario of the pass: validated, re-laid out, its union grid built; false: w.err says what is wrong with it
bool Upload::scenario(int r, UploadWorker &w)
{
    auto bad = [&](const char *fmt, size_t i, int v) {
        char buf[256];
        snprintf(buf, sizeof buf, fmt, i, v);
        w.err = buf;
        w.err_r = r;
        return false;
    };
    std::vector<double> &times = w.times, &merged = w.merged;
    if (sc->ego[r] < 0 || sc->ego[r] >= E) return bad("sg_upload: ego[%zu]=%d out of range", (size_t)r, sc->ego[r]);
    sstat[r].ego = sc->ego[r];
    if (sc->ego[r] != 0) w.ego_nz = 1;
    sstat[r].t0 = sc->t0[r];
    sstat[r].length = sc->length[r];
    for (int e = 0; e < EP; ++e) slot_defaults((size_t)r * EP + e);
    for (int e = 0; e < E; ++e) {
        size_t i = (size_t)r * E + e, o = (size_t)r * EP + e;
        int k = sc->kind[i];
        if (k < SG_KIND_NONE || k > SG_KIND_AGENT_EXTERNAL) return bad("sg_upload: kind[%zu]=%d unknown", i, k);
        if (k == SG_KIND_AGENT_EXTERNAL) ++w.ext_cnt;
        if (k == SG_KIND_AGENT_PEDESTRIAN) {
            int64_t ra = sc->route_off[i], rb = sc->route_off[i + 1];
            if (ra < 0 || rb <= ra) return bad("sg_upload: pedestrian agent %zu has no route (%d)", i, 0);
            SI(o, sg::ST_ROUTE) = ra | ((rb - ra) << 48);
        }
        int64_t a = sc->knot_off[i], b = sc->knot_off[i + 1];
        if (a < 0 || b < a || b > rows_total) return bad("sg_upload: knot_off not monotone at %zu (%d)", i, 0);
        if (k != SG_KIND_NONE && b == a) return bad("sg_upload: entity %zu has no knots (%d)", i, 0);
        SI(o, sg::ST_META) = (int64_t)k | ((int64_t)(sc->etype[i] & 0xff) << 8) | ((int64_t)(b - a) << 32);
        SI(o, sg::ST_KNOT_OFF) = a;
        for (int q = 0; q < 4; ++q) S(o, sg::ST_BW + q) = sc->bbox[i * 4 + q];
        if (sc->ctrl) for (int q = 0; q < sg::NCTRL_ROWS; ++q) S(o, sg::ST_CTRL + q) = sc->ctrl[i * SG_NCTRL + q];
        if (b > a) {
            S(o, sg::ST_MIN_T) = sc->knots[(size_t)a * 7];
            S(o, sg::ST_MAX_T) = sc->knots[(size_t)(b - 1) * 7];
            for (int64_t j = a + 1; j < b; ++j)
                if (!(sc->knots[(size_t)j * 7] > sc->knots[(size_t)(j - 1) * 7]))
                    return bad("sg_upload: knot times of entity %zu are not strictly increasing (%d)", i, 0);
            // the row is in cache: are z, pitch and roll +0.0 in every knot (bit patterns: -0.0 and NaN are not)?
            uint64_t any = 0;
            for (int64_t j = a; j < b; ++j) {
                const uint64_t *kr = reinterpret_cast<const uint64_t *>(sc->knots + (size_t)j * 7);
                any |= kr[3] | kr[5] | kr[6];
            }
            if (any) zpr_zero[r] = 0;
        }
    }
    // the union grid (np.unique of the concatenated knot times), while the scenario's knots are in cache.  Every
    // entity's times are strictly increasing (checked above), so the union grows by merging sorted lists -- and
    // an entity on the grid found so far (the usual case: one recording, one clock) costs one comparison per knot
    std::vector<double> &g = grids[r];
    for (int e = 0; e < E; ++e) {
        size_t i = (size_t)r * E + e;
        if (sc->kind[i] != SG_KIND_REPLAY) continue;
        const int64_t a = sc->knot_off[i], b = sc->knot_off[i + 1];
        const size_t n = (size_t)(b - a);
        if (n == 1) { // batch.py:85-88: a second knot 0.1 s later
            const double v0 = sc->knots[(size_t)a * 7], two[2] = {v0 == v0 ? v0 : 0.0 /* np.nan_to_num */, v0 + 1e-1};
            merged.clear();
            std::set_union(g.begin(), g.end(), two, two + 2, std::back_inserter(merged));
            g.swap(merged);
            continue;
        }
        bool same = g.size() == n;
        for (size_t j = 0; j < n && same; ++j) same = g[j] == sc->knots[(size_t)(a + (int64_t)j) * 7];
        if (same) continue;
        times.resize(n);
        for (size_t j = 0; j < n; ++j) times[j] = sc->knots[(size_t)(a + (int64_t)j) * 7];
        merged.clear();
        std::set_union(g.begin(), g.end(), times.begin(), times.end(), std::back_inserter(merged));
        g.swap(merged);
    }
    return true;
}

int Upload::host_pass()
{
    // scenarios are validated, re-laid out and given their union grid in parallel (the strictly-increasing check walks
    // every knot: 33 M for the 4096 x 64 x 128 batch; the grid sorts them); the first error by scenario index is reported
    const unsigned nthr = host_threads();
    std::vector<UploadWorker> ws(nthr);
    for (auto &w : ws) w.err_r = R;
    zpr_zero.assign(R, 1);
    auto work = [&](unsigned w) { // (a thread stops at the first scenario it cannot take)
        for (int r = (int)((int64_t)R * w / nthr); r < (int)((int64_t)R * (w + 1) / nthr); ++r)
            if (!scenario(r, ws[w])) return;
    };
    std::vector<std::thread> pool;
    for (unsigned w = 1; w < nthr; ++w) pool.emplace_back(work, w);
    work(0);
    for (auto &th : pool) th.join();
    unsigned first = 0;
    for (unsigned w = 1; w < nthr; ++w)
        if (ws[w].err_r < ws[first].err_r) first = w;
    if (ws[first].err_r < R) return fail(h, SG_ERR_INVALID, "%s", ws[first].err.c_str());
    for (unsigned w = 0; w < nthr; ++w) {
        n_ext += ws[w].ext_cnt;
        if (ws[w].ego_nz) h->ego_first = false;
    }
    // the controlled lanes in entity order (their index is the column of the controller table)
    for (int r = 0; r < R; ++r)
        for (int e = 0; e < E; ++e) {
            const int k = sc->kind[(size_t)r * E + e];
            if (k == SG_KIND_AGENT_PID || k == SG_KIND_AGENT_VEHICLE ||
                (h->crowd_riders && (k == SG_KIND_REPLAY || k == SG_KIND_AGENT_REPLAY))) {
                const size_t o = (size_t)r * EP + e;
                SI(o, sg::ST_CTL) = (int64_t)ctl_ent.size();
                ctl_ent.push_back((int32_t)o);
            }
        }
    return SG_OK;
}

// grid offsets, and the clocks
void Upload::lay_out_grids()
{
    grid_off.assign(R + 1, 0);
    for (int r = 0; r < R; ++r) {
        sstat[r].grid_n = (int32_t)grids[r].size();
        sstat[r].grid_off = grid_off[r];
        grid_off[r + 1] = grid_off[r] + sstat[r].grid_n;
    }
    total_rows = grid_off[R];
    grid_t.resize((size_t)total_rows);
    row_scen.resize((size_t)total_rows);
    for (int r = 0; r < R; ++r) {
        std::copy(grids[r].begin(), grids[r].end(), grid_t.begin() + grid_off[r]);
        std::fill(row_scen.begin() + grid_off[r], row_scen.begin() + grid_off[r + 1], r);
    }

    {   // scenarios that start at the same time run on the same clock (launch_sliced)
        std::vector<std::pair<uint64_t, int>> key(R);
        for (int r = 0; r < R; ++r) { uint64_t b; std::memcpy(&b, &sstat[r].t0, 8); key[r] = {b, r}; }
        std::sort(key.begin(), key.end());
        h->clock_t0.clear();
        h->clock_of.assign(R, 0);
        for (int i = 0; i < R; ++i) {
            if (i == 0 || key[i].first != key[i - 1].first) h->clock_t0.push_back(sstat[key[i].second].t0);
            h->clock_of[key[i].second] = (int)h->clock_t0.size() - 1;
        }
    }
}

// the device copies of what does not change while the batch runs
int Upload::static_arrays()
{
    // ---- device copies ----
    p = Params{};
    p.R = R; p.E = E; p.EP = EP;
    p.WV = h->WV; p.FROWS = SG_F_COLL + h->WV;
    p.sf = h->sf;
    p.ped_behaviour = h->ped_behaviour;
    p.n_ped_models = h->n_ped_models;
    p.ped_models = h->d_ped_models;
    p.model_of = h->d_model_of;
    apply_noise(h);
    p.ped_serial = h->ped_serial;
    p.ctl_general = env_int("SG_CTL_FAST", 1) == 0;
    p.quiet = h->quiet;
    p.reset_mask = h->d_reset_mask;
    p.persist = h->cfg.persist;
    p.term_mask = h->cfg.terminal_mask;
    p.rec_cap = h->cfg.record_capacity > 0 ? h->cfg.record_capacity : 0;
    p.ev_cap = h->cfg.event_capacity > 0 ? h->cfg.event_capacity : 0;
    auto &SA = h->static_allocs;
    int rc = 0;
    {
        double *d_stat = nullptr;
        if ((rc = dev_alloc(h, SA, &d_stat, stat_n, false))) return rc;
        HIP_TRY(h, hipMemcpyAsync(d_stat, stat, stat_n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        p.stat = d_stat;
    }
    if ((rc = dev_upload(h, SA, &p.sstat, sstat))) return rc;
    if ((rc = dev_upload(h, SA, &p.grid_t, grid_t))) return rc;
    {
        p.knots = d_knots; // (on its way since start_knot_copy)
        const int32_t *drs = nullptr;
        if ((rc = dev_upload(h, SA, &drs, row_scen))) return rc;
        h->d_row_scen = const_cast<int32_t *>(drs);
        h->total_rows = total_rows;
        if ((rc = dev_alloc(h, SA, &p.grid_y, (size_t)total_rows * 6 * EP, false))) return rc;
    }
    {   // pedestrian routes + the 64-gon table of Point.buffer (host libm, as shapely's caller sees it)
        size_t rrows = sc->route_off ? (size_t)sc->route_off[(size_t)R * E] : 0;
        std::vector<double> routes(sc->routes, sc->routes + rrows * 2);
        if (routes.empty()) routes.assign(2, 0.0);
        if ((rc = dev_upload(h, SA, &p.routes, routes))) return rc;
        std::vector<double> gon(128);
        for (int i = 0; i < 64; ++i) { double a = 2.0 * 3.141592653589793 * i / 64; gon[2 * i] = std::cos(a); gon[2 * i + 1] = std::sin(a); }
        if ((rc = dev_upload(h, SA, &p.gon, gon))) return rc;
    }
    h->n_ext = n_ext;
    {   // external poses start as "None" (NaN: all-ones bytes) for every slot
        double *d = nullptr;
        if ((rc = dev_alloc(h, SA, &d, NE * 6, false))) return rc;
        HIP_TRY(h, hipMemsetAsync(d, 0xFF, NE * 6 * sizeof(double), h->stream));
        h->d_ext = d;
        p.ext_pose = d;
    }
    h->n_ctl = (int)ctl_ent.size();
    h->max_ctl_per_block = 0;
    for (size_t i = 0, run = 0; i < ctl_ent.size(); ++i) { // ctl_ent is sorted by entity index
        run = (i > 0 && (ctl_ent[i] >> 6) == (ctl_ent[i - 1] >> 6)) ? run + 1 : 1;
        h->max_ctl_per_block = std::max(h->max_ctl_per_block, (int)run);
    }
    h->planar = n_ext == 0 && env_int("SG_PLANAR", 1) != 0; // (the table variant of the rollout kernel: rollout_kernel_tab_planar)
    for (int r = 0; r < R && h->planar; ++r) h->planar = zpr_zero[r] != 0;
    ctl_ent.resize(((ctl_ent.size() + 63) / 64) * 64, -1);
    p.n_ctl_pad = (int)ctl_ent.size();
    if ((rc = dev_upload(h, SA, &p.ctl_ent, ctl_ent))) return rc;
    return SG_OK;
}

// ... and of what a rollout writes
int Upload::state_arrays()
{
    auto &M = h->state_allocs;
    int rc = 0;
    if ((rc = dev_alloc(h, M, &p.ctl_state, (size_t)sg::CS_COUNT * std::max(p.n_ctl_pad, 1)))) return rc;
    if ((rc = dev_alloc(h, M, &p.dyn, nblk * (size_t)p.FROWS * 64))) return rc;
    if ((rc = dev_alloc(h, M, &p.sdyn, (size_t)R))) return rc;
    if ((rc = dev_alloc(h, M, &p.events, (size_t)R * std::max(p.ev_cap, 1)))) return rc;
    if ((rc = dev_alloc(h, M, &p.ev_pose, (size_t)R * std::max(p.ev_cap, 1) * 3))) return rc;
    if ((rc = dev_alloc(h, M, &p.ev_hpose, (size_t)R * std::max(p.ev_cap, 1) * 3, false))) return rc;
    HIP_TRY(h, hipMemsetAsync(p.ev_hpose, 0xFF, (size_t)R * std::max(p.ev_cap, 1) * 3 * sizeof(double), h->stream));
    if ((rc = dev_alloc(h, M, &p.rec_t, (size_t)std::max(p.rec_cap, 1) * R))) return rc;
    if ((rc = dev_alloc(h, M, &p.rec_pose, (size_t)std::max(p.rec_cap, 0) * 6 * R * EP + 1))) return rc;

#ifdef SG_PHASE_TIMERS
    if ((rc = dev_alloc(h, M, &p.phase_cycles, 16 + 4096))) return rc;
#endif
    return SG_OK;
}

int Upload::resample()
{
    // stage-1 resample on the device, piece by piece behind the knot copy
    for (int c = 0; c < UP_CHUNKS; ++c) {
        while (issued.load(std::memory_order_acquire) <= c) std::this_thread::yield();
        const int64_t row0 = grid_off[chunk_r[c]], row1 = grid_off[chunk_r[c + 1]];
        if (rows_total <= 0 || row1 <= row0) continue;
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->up_ev[c], 0));
        const int64_t threads = (row1 - row0) * EP;
        sgl::build_grid(dim3((unsigned)((threads + 255) / 256)), h->stream, p, h->d_row_scen, row0, row1);
        HIP_TRY(h, hipGetLastError());
    }
    copier.join();
    if (copy_err != hipSuccess) return fail(h, SG_ERR_HIP, "sg_upload: copying the knots failed: %s", hipGetErrorString(copy_err));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // host vectors go out of scope
    return SG_OK;
}
} // namespace

extern "C" int sg_upload(sg_handle *h, const sg_scenarios *sc)
{
    if (!h || !sc) return SG_ERR_INVALID;
    if (!sc->kind || !sc->etype || !sc->bbox || !sc->knot_off || !sc->knots || !sc->ego || !sc->t0 || !sc->length)
        return fail(h, SG_ERR_INVALID, "sg_upload: null array in sg_scenarios");
    const auto t_entry = std::chrono::steady_clock::now();
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    forget_queue_failure(h);
    HIP_TRY(h, hipStreamSynchronize(h->ctl_stream));
    forget_batch(h);
    int rc = classify_batch(h, sc);
    if (rc) return rc;
    Upload u(h, sc, t_entry);
    u.stage("entry (syncs, pools, kinds)");
    if ((rc = u.start_knot_copy()) || (rc = u.stat_buffer()) || (rc = u.host_pass())) return rc;
    u.stage("validate + re-layout + union grids");
    u.lay_out_grids();
    u.stage("union grids");
    if ((rc = u.static_arrays()) || (rc = u.state_arrays()) || (rc = u.resample())) return rc;
    u.stage("knot copy (since the start) + stage-1 resample");
    h->uploaded = true;
    int rc_reset = sg_reset(h);
    u.stage("reset");
    return rc_reset;
}

extern "C" int sg_reset(sg_handle *h)
{
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_reset: no scenarios uploaded");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    bool fused = false;
    int rc = rss_fused_call(h, false, &fused);
    if (!rc) rc = launch_rollout(h, 0, 1, 0, nullptr, fused);
    if (!rc && h->rss_enabled && !fused) rc = sg_rss_update(h, 1);
    if (rc) return rc;
    forget_episodes(h); // (a new episode for everybody: the accounting of sg_tick_drivers starts anew)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SG_OK;
}

extern "C" int sg_reset_scenarios(sg_handle *h, const uint8_t *mask)
{
    if (!h || !mask) return h ? fail(h, SG_ERR_INVALID, "sg_reset_scenarios: null mask") : SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_reset_scenarios: no scenarios uploaded");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->d_reset_mask) HIP_TRY(h, hipMalloc((void **)&h->d_reset_mask, (size_t)h->R));
    HIP_TRY(h, hipMemcpyAsync(h->d_reset_mask, mask, (size_t)h->R, hipMemcpyHostToDevice, h->stream));
    if (const int rc = reset_scenarios_queued(h, h->d_reset_mask, true)) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SG_OK;
}

// (the reset launch reads its mask from device memory, Params::reset_mask, whoever filled it)
int sgh::reset_scenarios_queued(sg_handle *h, const uint8_t *d_mask, bool clear_episodes)
{
    h->p.reset_mask = d_mask;
    bool fused = false; // (the flagged scenarios' RSS histories start anew as well)
    int rc = rss_fused_call(h, true, &fused);
    if (!rc) rc = launch_rollout(h, 0, 2, 0, nullptr, fused);
    if (!rc && clear_episodes) rc = episode_clear_masked(h, d_mask);
    return rc;
}

extern "C" int sg_reset_scenarios_device(sg_handle *h, const uint8_t *d_mask)
{
    if (!h || !d_mask) return h ? fail(h, SG_ERR_INVALID, "sg_reset_scenarios_device: null mask") : SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_reset_scenarios_device: no scenarios uploaded");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return reset_scenarios_queued(h, d_mask, true);
}

extern "C" int sg_set_external_poses(sg_handle *h, const double *poses)
{
    if (!h || !poses) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_set_external_poses: no scenarios uploaded");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t row = (size_t)h->E * 6 * sizeof(double);
    if (h->EP == h->E) {
        HIP_TRY(h, hipMemcpyAsync(h->d_ext, poses, (size_t)h->R * row, hipMemcpyHostToDevice, h->stream));
    } else { // padded entity stride on the device
        HIP_TRY(h, hipMemcpy2DAsync(h->d_ext, (size_t)h->EP * 6 * sizeof(double), poses, row, row, (size_t)h->R,
                                    hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // the caller's buffer is free on return
    return SG_OK;
}
