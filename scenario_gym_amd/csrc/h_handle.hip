// h_handle.hip -- the handle of the C ABI: creation and destruction, the small setters, the statistics of the last call.
#include "sgym_host.hpp"

using namespace sgh;

thread_local std::string sgh::g_create_err;

int sgh::fail(sg_handle *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_err = buf;
    return code;
}

int sgh::GrowBuf::ensure(sg_handle *h, size_t bytes, bool *grew)
{
    if (grew) *grew = false;
    if (bytes <= cap) return SG_OK;
    if (ptr) HIP_TRY(h, kind == HOST ? hipHostFree(ptr) : hipFree(ptr));
    ptr = nullptr;
    cap = 0;
    HIP_TRY(h, kind == HOST ? hipHostMalloc(&ptr, bytes, hipHostMallocDefault) : hipMalloc(&ptr, bytes));
    if (kind == DEVICE_POISONED) poison(h->stream, ptr, bytes);
    cap = bytes;
    if (grew) *grew = true;
    return SG_OK;
}

void sgh::GrowBuf::release()
{
    if (ptr) (void)(kind == HOST ? hipHostFree(ptr) : hipFree(ptr));
    ptr = nullptr;
    cap = 0;
}

extern "C" int sg_version(void) { return SG_ABI_VERSION; }

extern "C" const char *sg_last_error(const sg_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int sg_create(const sg_config *cfg, sg_handle **out)
{
    if (!cfg || !out) return fail(nullptr, SG_ERR_INVALID, "sg_create: null argument");
    *out = nullptr;
    if (cfg->n_scenarios <= 0 || cfg->n_entities <= 0)
        return fail(nullptr, SG_ERR_INVALID, "sg_create: n_scenarios and n_entities must be positive");
    if (cfg->n_entities > 16384)
        return fail(nullptr, SG_ERR_INVALID, "sg_create: n_entities=%d > 16384 (the event record keeps the other entity in 32 bits, "
                    "the state blocks SG_F_COLL + n_entities / 64 rows: nothing stops at 512 any more, this is a sanity bound)",
                    cfg->n_entities);
    if (!(cfg->timestep > 0.0)) return fail(nullptr, SG_ERR_INVALID, "sg_create: timestep must be > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, SG_ERR_NO_DEVICE, "sg_create: no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, SG_ERR_INVALID, "sg_create: device %d out of range (%d devices)", cfg->device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, SG_ERR_HIP, "sg_create: hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, SG_ERR_NO_DEVICE, "sg_create: device %d is %s; this library is built for gfx950 only",
                    cfg->device, prop.gcnArchName);
    sg_handle *h = new sg_handle();
    h->cfg = *cfg;
    h->R = cfg->n_scenarios;
    h->E = cfg->n_entities;
    int G = 4;
    while (G < h->E && G < 64) G <<= 1;
    h->G = G;
    // wavefronts per scenario.  8 (257..512 entities): the eight-wavefront instances of the general variants (plain, pedestrian,
    // RSS, road); the table path, the crowd kernels and the riders' pre-pass stop at 256.
    // More than 512: no fused kernel -- the step runs as four kernels over as many workgroups as the scenario needs (sgym_wide.hpp)
    h->WV = h->E <= 64 ? 1 : (h->E <= 128 ? 2 : (h->E <= 256 ? 4 : (h->E <= 512 ? 8 : (h->E + 63) / 64)));
    h->wide = h->WV > 8;
    if (h->wide && h->R > 65535) { // (the scenario is the y coordinate of the wide kernels' grids)
        delete h;
        return fail(nullptr, SG_ERR_INVALID, "sg_create: more than 65535 scenarios of more than 512 entities in one handle (n_scenarios=%d)", cfg->n_scenarios);
    }
    h->EP = G * h->WV;
    // SocialForceParameters defaults, pedestrian/social_force.py:16-30 (noise off)
    h->sf = sg_social_force{1.5, 1.0, 1.0, 0.0, 0.5, 1.0, std::cos(200.0 / 2 * M_PI / 180), 1.3, 0.0, 0.0, 2.0, 0.1};
    h->NE = (((size_t)h->R * h->EP + 63) / 64) * 64;
    h->tab_min = env_int("SG_TAB_MIN_STEPS", h->tab_min);
    h->chunk_steps = env_int("SG_CHUNK_STEPS", h->chunk_steps);
    h->overlap = env_int("SG_OVERLAP", h->overlap);
    h->ctl_slice = std::max(1, env_int("SG_CTL_SLICE", h->ctl_slice));
    h->ped_serial = env_int("SG_PED_SERIAL", 0) != 0;
    h->crowd_kernel = env_int("SG_CROWD_KERNEL", 1);
    h->crowd_models = env_int("SG_CROWD_MODELS", 1) != 0; // (0: batches with several pedestrian models keep to the general variant; the tests compare)
    h->slice_mode = env_int("SG_SLICE", 1);
    h->queue_mode = env_int("SG_QUEUE", 1);
    h->quiet = env_int("SG_QUIET", 1) != 0;
    h->snap_d2d = env_int("SG_SNAP_D2D", 0); // (tools/snapshot_time.py compares the two)
    // the controller stream carries the serial chain of the table path (control_kernel_fast: 64 wavefronts that every rollout
    // launch waits for): highest stream priority, so that its launches are dispatched ahead of the rollout kernels'
    // (measured: no difference at 4096 x 64, where the launches never queue; SG_CTL_PRIO=0 creates it at the lowest)
    int prio_lo = 0, prio_hi = 0;
    if (hipSetDevice(cfg->device) != hipSuccess || hipStreamCreate(&h->stream) != hipSuccess ||
        hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess ||
        hipStreamCreateWithPriority(&h->ctl_stream, hipStreamNonBlocking * 0, env_int("SG_CTL_PRIO", 1) ? prio_hi : prio_lo) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
        delete h;
        return fail(nullptr, SG_ERR_HIP, "sg_create: stream/event creation failed");
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) h->n_simd = 4 * cus;
        else (void)hipGetLastError();
    }
    *out = h;
    return SG_OK;
}

extern "C" int sg_destroy(sg_handle *h)
{
    if (!h) return SG_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
#ifdef SG_RSS_STATS
    {
        unsigned long long c[8];
        (void)hipMemcpyFromSymbol(c, HIP_SYMBOL(sg::sg_rss_stats), sizeof c);
        fprintf(stderr, "rss stats: flushes %llu groups %llu items %llu passes %llu wave-updates %llu lat-lanes %llu long-lanes %llu\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6]);
    }
#endif
#ifdef SG_PHASE_TIMERS
    if (h->p.phase_cycles) {
        unsigned long long c[16];
        (void)hipMemcpy(c, h->p.phase_cycles, sizeof c, hipMemcpyDeviceToHost);
        unsigned long long tot = 0;
        for (int i = 0; i < 16; ++i) tot += c[i];
        fprintf(stderr, "phase cycles (s_memtime, summed over wavefronts):");
        for (int i = 0; i < 16; ++i) fprintf(stderr, " [%d] %.1f%%", i, tot ? 100.0 * c[i] / tot : 0.0);
        fprintf(stderr, "  total %.3e\n", (double)tot);
        std::vector<unsigned long long> hw(4096);
        (void)hipMemcpy(hw.data(), h->p.phase_cycles + 16, 4096 * 8, hipMemcpyDeviceToHost);
        for (int b = 0; b < 12; ++b) {
            fprintf(stderr, "block %d:", b);
            for (int w = 0; w < 4; ++w) { unsigned v = (unsigned)hw[b * 4 + w]; fprintf(stderr, " [wave %u simd %u cu %u se %u xcc?%x]", v & 15, (v >> 4) & 3, (v >> 8) & 15, (v >> 13) & 7, v >> 16); }
            fprintf(stderr, "\n");
        }
    }
#endif
    free_snapshots(h);
    free_pool(h->static_allocs);
    free_pool(h->state_allocs);
    free_pool(h->road_allocs);
    free_pool(h->lane_allocs);
    free_pool(h->slice_allocs);
    free_pool(h->wide_allocs);
    h->pin_sd.release();
    h->pin_ev.release();
    h->obs.release();
    h->road_info.release();
    h->observers.release();
    h->routes.release();
    h->drivers.release();
    h->drv_actions.release();
    h->policy.release();
    h->pol_actions.release();
    h->pol_out.release();
    h->episode.release();
    if (h->d_reset_mask) (void)hipFree(h->d_reset_mask);
    h->term_flags.release();
    if (h->d_rss_state) (void)hipFree(h->d_rss_state);
    if (h->d_rss_seen) (void)hipFree(h->d_rss_seen);
    if (h->d_rss_code) (void)hipFree(h->d_rss_code);
    if (h->d_rss_safe) (void)hipFree(h->d_rss_safe);
    if (h->d_rssq) (void)hipFree(h->d_rssq);
    if (h->d_rssq_n) (void)hipFree(h->d_rssq_n);
    if (h->tick_exec) (void)hipGraphExecDestroy(h->tick_exec);
    if (h->ctl_stream) (void)hipStreamSynchronize(h->ctl_stream);
    h->actions.release();
    if (h->d_gon) (void)hipFree(h->d_gon);
    if (h->d_normals) (void)hipFree(h->d_normals);
    for (int b = 0; b < 4; ++b)
        if (h->d_tab[b]) (void)hipFree(h->d_tab[b]);
    if (h->d_ped_models) (void)hipFree(h->d_ped_models);
    if (h->d_model_of) (void)hipFree(h->d_model_of);
    h->qwords.release();
    if (h->d_qtab) (void)hipFree(h->d_qtab);
    if (h->q_host) (void)hipHostFree(h->q_host);
    if (h->wide_running) (void)hipHostFree(h->wide_running);
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->up_ev) (void)hipEventDestroy(e);
    h->up_stat.release();
    if (h->ctl_stream) (void)hipStreamDestroy(h->ctl_stream);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SG_OK;
}

extern "C" int sg_set_timestep(sg_handle *h, double timestep)
{
    if (!h || !(timestep > 0.0)) return h ? fail(h, SG_ERR_INVALID, "sg_set_timestep: timestep must be > 0") : SG_ERR_INVALID;
    h->cfg.timestep = timestep;
    ++h->generation;
    return SG_OK;
}

extern "C" void *sg_stream(sg_handle *h) { return h ? (void *)h->stream : nullptr; }

extern "C" int sg_copy_to_host(sg_handle *h, const void *device_ptr, void *host_ptr, uint64_t bytes)
{
    if (!h || !device_ptr || !host_ptr) return SG_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(host_ptr, device_ptr, bytes, hipMemcpyDeviceToHost));
    return check_queue(h);
}

extern "C" int sg_last_kernel_ms(sg_handle *h, float *ms)
{
    if (!h || !ms) return SG_ERR_INVALID;
    if (!h->timed) return fail(h, SG_ERR_STATE, "sg_last_kernel_ms: the last call was not timed (nothing launched yet, or fewer than 16 steps)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    HIP_TRY(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return SG_OK;
}

// (start, end) of the hot-path launches of the last timed call, ms after the call's first event
static int launch_intervals(sg_handle *h, std::vector<std::pair<float, float>> &iv)
{
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    iv.clear();
    for (int i : h->launch_ev) {
        float a = 0.0f, d = 0.0f;
        HIP_TRY(h, hipEventElapsedTime(&a, h->ev0, h->ev_pool[i]));
        HIP_TRY(h, hipEventElapsedTime(&d, h->ev_pool[i], h->ev_pool[i + 1]));
        iv.emplace_back(a, a + d);
    }
    return SG_OK;
}

extern "C" int sg_last_launch_stats(sg_handle *h, int32_t *n_launches, float *kernel_ms_total)
{
    if (!h || !n_launches || !kernel_ms_total) return SG_ERR_INVALID;
    if (!h->timed) return fail(h, SG_ERR_STATE, "sg_last_launch_stats: the last call was not timed (nothing launched yet, or fewer than 16 steps)");
    std::vector<std::pair<float, float>> iv;
    int rc = launch_intervals(h, iv);
    if (rc) return rc;
    // the union of the launches' intervals: launches of the two pipelines overlap (launch_rollout), time counts once
    std::sort(iv.begin(), iv.end());
    float total = 0.0f, lo = 0.0f, hi = -1.0f;
    for (const auto &x : iv) {
        if (hi < lo || x.first > hi) {
            if (hi >= lo) total += hi - lo;
            lo = x.first;
            hi = x.second;
        } else {
            hi = std::max(hi, x.second);
        }
    }
    if (hi >= lo) total += hi - lo;
    *n_launches = h->n_launches;
    *kernel_ms_total = total;
    return SG_OK;
}

extern "C" const char *sg_last_kernel(sg_handle *h) { return h ? h->last_kernel : ""; }

extern "C" int sg_schedule_info(sg_handle *h, int32_t *info)
{
    if (!h || !info) return SG_ERR_INVALID;
    info[0] = h->last_schedule;
    info[1] = h->last_schedule == 2 ? h->last_chunks : 0;
    info[2] = h->last_schedule == 2 ? h->last_ring : 0;
    info[3] = h->last_schedule == 2 ? h->last_grid : 0;
    info[4] = h->p.n_ctl_pad / 64;
    info[5] = (int32_t)std::min<size_t>(0x7fffffff, h->NE / 64);
    info[6] = h->n_simd;
    info[7] = h->n_launches;
    return SG_OK;
}

extern "C" int sg_last_launch_gross_ms(sg_handle *h, float *kernel_ms_gross)
{
    if (!h || !kernel_ms_gross) return SG_ERR_INVALID;
    if (!h->timed) return fail(h, SG_ERR_STATE, "sg_last_launch_gross_ms: the last call was not timed (nothing launched yet, or fewer than 16 steps)");
    std::vector<std::pair<float, float>> iv;
    int rc = launch_intervals(h, iv);
    if (rc) return rc;
    float total = 0.0f;
    for (const auto &x : iv) total += x.second - x.first;
    *kernel_ms_gross = total;
    return SG_OK;
}

extern "C" int sg_debug_trig32(sg_handle *h, int64_t n, const double *heading, float *sin_out, float *cos_out)
{
    if (!h || n < 0 || !heading || !sin_out || !cos_out) return SG_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    double *d_h = nullptr;
    float *d_s = nullptr, *d_c = nullptr;
    const size_t m = (size_t)std::max<int64_t>(n, 1);
    HIP_TRY(h, hipMalloc((void **)&d_h, m * sizeof(double)));
    HIP_TRY(h, hipMalloc((void **)&d_s, m * sizeof(float)));
    HIP_TRY(h, hipMalloc((void **)&d_c, m * sizeof(float)));
    int rc = SG_OK;
    do {
        if (hipMemcpy(d_h, heading, (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { rc = SG_ERR_HIP; break; }
        if (n > 0) sgl::trig32(dim3((unsigned)((n + 255) / 256)), h->stream, d_h, d_s, d_c, n);
        if (hipStreamSynchronize(h->stream) != hipSuccess) { rc = SG_ERR_HIP; break; }
        if (hipMemcpy(sin_out, d_s, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { rc = SG_ERR_HIP; break; }
        if (hipMemcpy(cos_out, d_c, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { rc = SG_ERR_HIP; break; }
    } while (0);
    (void)hipFree(d_h); (void)hipFree(d_s); (void)hipFree(d_c);
    if (rc) return fail(h, rc, "sg_debug_trig32: HIP copy/launch failed");
    return SG_OK;
}

extern "C" int sg_host_alloc(int32_t device, uint64_t bytes, void **out)
{
    if (!out || bytes == 0) return SG_ERR_INVALID;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return SG_ERR_HIP;
    return hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault) == hipSuccess ? SG_OK : SG_ERR_HIP;
}

extern "C" int sg_host_free(void *p)
{
    if (!p) return SG_OK;
    return hipHostFree(p) == hipSuccess ? SG_OK : SG_ERR_HIP;
}

extern "C" int sg_set_slicing(sg_handle *h, int32_t mode)
{
    if (!h || mode < 0 || mode > 2) return h ? fail(h, SG_ERR_INVALID, "sg_set_slicing: mode 0, 1 or 2") : SG_ERR_INVALID;
    h->slice_mode = mode;
    return SG_OK;
}

extern "C" int sg_set_tuning(sg_handle *h, int32_t tab_min_steps, int32_t chunk_steps, int32_t overlap)
{
    if (!h) return SG_ERR_INVALID;
    if (tab_min_steps >= 0) h->tab_min = tab_min_steps;
    if (chunk_steps > 0) h->chunk_steps = chunk_steps;
    if (overlap >= 0) h->overlap = overlap != 0;
    ++h->generation;
    return SG_OK;
}

extern "C" int sg_set_collision_tolerance(sg_handle *h, double c_tol)
{
    if (!h || !(c_tol >= 0.0)) return h ? fail(h, SG_ERR_INVALID, "sg_set_collision_tolerance: c_tol must be >= 0") : SG_ERR_INVALID;
    h->c_tol = c_tol;
    return SG_OK;
}
