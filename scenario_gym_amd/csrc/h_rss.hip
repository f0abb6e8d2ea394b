// h_rss.hip -- RSSDistances: the records and the line-test queue of a handle, the callback as a launch of its own.
#include "sgym_host.hpp"

using namespace sgh;

// the RSS record arrays of the current batch (freed by sg_upload); returns 1 in *fresh when they were just created
int sgh::ensure_rss(sg_handle *h, bool *fresh)
{
    *fresh = false;
    if (h->d_rss_state && h->rss_NE != h->NE) { // (another padded entity count: sg_upload of a pedestrian batch narrower than 16)
        (void)hipFree(h->d_rss_state); (void)hipFree(h->d_rss_code); (void)hipFree(h->d_rss_safe); (void)hipFree(h->d_rss_seen);
        h->d_rss_state = nullptr; h->d_rss_code = nullptr; h->d_rss_safe = nullptr; h->d_rss_seen = nullptr;
    }
    if (!h->d_rss_state) {
        HIP_TRY(h, hipMalloc((void **)&h->d_rss_state, h->NE * sizeof(int32_t)));
        HIP_TRY(h, hipMalloc((void **)&h->d_rss_code, h->NE * sizeof(int32_t)));
        HIP_TRY(h, hipMalloc((void **)&h->d_rss_safe, h->NE * 2 * sizeof(double)));
        HIP_TRY(h, hipMalloc((void **)&h->d_rss_seen, (size_t)h->R * sizeof(int32_t)));
        h->rss_NE = h->NE;
        h->rss_stale = true;
    }
    if (h->rss_stale) { // first use after sg_create / sg_upload: the records of a new batch
        HIP_TRY(h, hipMemsetAsync(h->d_rss_state, 0, h->NE * sizeof(int32_t), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->d_rss_code, 0xff, h->NE * sizeof(int32_t), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->d_rss_safe, 0xff, h->NE * 2 * sizeof(double), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->d_rss_seen, 0xff, (size_t)h->R * sizeof(int32_t), h->stream));
        h->rss_stale = false;
        *fresh = true;
    }
    h->p.rss_state = h->d_rss_state; h->p.rss_code = h->d_rss_code; h->p.rss_safe = h->d_rss_safe; h->p.rss_seen = h->d_rss_seen;
    return SG_OK;
}

int sgh::ensure_rssq(sg_handle *h)
{
    if (h->wide) return SG_OK; // (scenarios of more than 512 entities run the callback as a launch of its own: no line-test queue)
    if (h->d_rssq && h->rssq_NE != h->NE) {
        (void)hipFree(h->d_rssq); (void)hipFree(h->d_rssq_n);
        h->d_rssq = nullptr; h->d_rssq_n = nullptr;
    }
    if (!h->d_rssq) {
        h->rssq_NE = h->NE;
        const size_t nw = h->NE / 64, per_step = nw * 64 * sg::RSSQ_REC * sizeof(double);
        // (SG_RSSQ_MB; default: an eighth of the free device memory, at least 4 GiB -- every launch boundary costs the tail of a
        // launch, and 288 GB hold the queues of a whole 1000-step rollout of the largest batches)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
        const int mb = env_int("SG_RSSQ_MB", 0);
        const size_t budget = mb > 0 ? (size_t)mb << 20 : std::max<size_t>((size_t)4096 << 20, free_b / 8);
        const int cap = std::max(1, env_int("SG_RSSQ_STEPS", 1024));
        int steps = (int)std::min<size_t>((size_t)cap, std::max<size_t>(2, budget / per_step) - 1);
        // the queue only sets how many steps one launch covers: when the device is short of memory, shorter launches
        //  instead of a failed sg_upload / sg_reset
        for (;; steps = std::max(1, steps / 2)) {
            const hipError_t e = hipMalloc((void **)&h->d_rssq, per_step * (size_t)(steps + 1));
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            h->d_rssq = nullptr;
            if (steps == 1) return fail(h, SG_ERR_HIP, "sg_set_rss: no device memory for the line-test queue (%zu bytes per step)", per_step);
        }
        HIP_TRY(h, hipMalloc((void **)&h->d_rssq_n, nw * sizeof(int32_t)));
        HIP_TRY(h, hipMemsetAsync(h->d_rssq_n, 0, nw * sizeof(int32_t), h->stream));
        h->rssq_steps = steps;
    }
    h->p.rssq = h->d_rssq; h->p.rssq_n = h->d_rssq_n; h->p.rssq_cap = (h->rssq_steps + 1) * 64;
    return SG_OK;
}

// RSSDistances.__call__ as a launch of its own (no fused variant carries it: plan_call's rss_alone)
void sgh::launch_rss_alone(sg_handle *h, int reset)
{
    sgl::rss(dim3((unsigned)h->R), dim3(512), h->stream, h->p, reset, h->d_rss_state, h->d_rss_code, h->d_rss_safe, h->d_rss_seen);
}

extern "C" int sg_rss_update(sg_handle *h, int32_t reset)
{
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_rss_update: no scenarios uploaded");

    if (!h->ego_first) return fail(h, SG_ERR_STATE, "sg_rss_update: RSSDistances keeps its records for entities[1:], the ego has to be entity 0 of every scenario");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    bool fresh = false;
    int rc0 = ensure_rss(h, &fresh);
    if (rc0) return rc0;
    if (fresh) reset = 1;
    sgl::rss(dim3((unsigned)h->R), dim3(h->EP > 256 ? 512 : 256), h->stream, h->p, reset ? 1 : 0, h->d_rss_state, h->d_rss_code, h->d_rss_safe, h->d_rss_seen);
    HIP_TRY(h, hipGetLastError());
    return SG_OK;
}

extern "C" int sg_set_rss(sg_handle *h, int32_t enabled)
{
    if (!h) return SG_ERR_INVALID;
    h->rss_enabled = enabled != 0;
    return SG_OK;
}

extern "C" int sg_rss_read(sg_handle *h, uint8_t *flags, int32_t *codes, double *safe)
{
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded || !rss_live(h)) return fail(h, SG_ERR_STATE, "sg_rss_read: sg_rss_update has not run on this batch");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (const int rcq = check_queue(h)) return rcq; // (a persistent launch that gave up: sticky)
    const int R = h->R, E = h->E, EP = h->EP;
    std::vector<int32_t> st(h->NE), cd(h->NE);
    std::vector<double> sf(h->NE * 2);
    HIP_TRY(h, hipMemcpy(st.data(), h->d_rss_state, h->NE * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (codes) HIP_TRY(h, hipMemcpy(cd.data(), h->d_rss_code, h->NE * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (safe) HIP_TRY(h, hipMemcpy(sf.data(), h->d_rss_safe, h->NE * 2 * sizeof(double), hipMemcpyDeviceToHost));
    for (int r = 0; r < R; ++r) {
        uint8_t f = 3;
        for (int e = 0; e < E; ++e) {
            const size_t i = (size_t)r * EP + e, o = (size_t)r * E + e;
            if ((st[i] & 0xff) == 2) f &= ~1u; // some entity's history holds "unsafe_longitudinal", rss.py:70-86
            if ((st[i] & 0xff) == 1) f &= ~2u;
            if (codes) codes[o] = cd[i];
            if (safe) { safe[o * 2] = sf[i * 2]; safe[o * 2 + 1] = sf[i * 2 + 1]; }
        }
        if (flags) flags[r] = f;
    }
    return SG_OK;
}
