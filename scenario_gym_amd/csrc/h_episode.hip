// h_episode.hip -- the multi-agent tick on the device (sg_tick_drivers): the step of the drivers (drivers_step, h_drive.hip), the
// terminal conditions, the drivers' status and route rows, episode_kernel (sgym_episode.hpp) and the auto-reset, one behind the other
// on the handle's stream; the buffer that holds the episode accounting and the arrays of sg_episode_view.
#include "sgym_host.hpp"

using namespace sgh;

// Lays the buffer out for the current driver list: the accounting at the front (doubles, ints, bytes: one memset zeroes it), then the
// arrays of the view, the widest element type first so that every array is aligned.  Only a change of the number of drivers moves
// anything (sg_set_drivers has waited for the stream by then).  The lengths and the prev_ok bytes each end on a multiple of 8, so
// that no 8-byte word holds cells of two arrays (snapshot_copy_kernel moves such cells as whole words).
int sgh::episode_layout(sg_handle *h)
{
    const size_t n = (size_t)h->drivers.n, R = (size_t)h->R;
    if (h->ep_n == h->drivers.n && h->episode.ptr) return SG_OK;
    const auto pad8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
    const size_t state = 2 * n * sizeof(double) + pad8(R * sizeof(int32_t)) + pad8(n);
    const size_t doubles = R + n * (SG_ST_NFEAT + SG_RT_NFEAT + 3), ints = 2 * R + n * (1 + SG_ST_NINFO + SG_RT_NINFO), bytes = 2 * R + n;
    const size_t total = state + doubles * sizeof(double) + ints * sizeof(int32_t) + bytes;
    h->ep_n = -1;
    forget_episodes(h);
    if (total > h->episode.cap) HIP_TRY(h, hipStreamSynchronize(h->stream)); // (a queued tick may still write the old buffer)
    if (const int rc = h->episode.ensure(h, total)) return rc;
    unsigned char *at = h->episode.as<unsigned char>();
    const auto take = [&](auto *&ptr, size_t count) {
        ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(at);
        at += count * sizeof(*ptr);
    };
    sg::EpisodeArgs &a = h->ep;
    sg_episode_view &v = h->ep_view;
    double *env_reward, *drv_feat, *drv_route;
    uint32_t *term_flags, *drv_flags;
    int32_t *drv_info, *drv_route_info;
    take(a.prev_s, n); take(a.acc_return, n); take(a.acc_length, R);
    at = h->episode.as<unsigned char>() + 2 * n * sizeof(double) + pad8(R * sizeof(int32_t));
    take(a.prev_ok, n);
    at = h->episode.as<unsigned char>() + state;
    take(env_reward, R); take(drv_feat, n * SG_ST_NFEAT); take(drv_route, n * SG_RT_NFEAT);
    take(a.drv_progress, n); take(a.drv_reward, n); take(a.ep_return, n);
    take(term_flags, R); take(a.ep_length, R); take(drv_flags, n); take(drv_info, n * SG_ST_NINFO); take(drv_route_info, n * SG_RT_NINFO);
    take(a.env_done, R); take(a.reset_mask, R); take(a.drv_done, n);
    assert(at == h->episode.as<unsigned char>() + total);
    a.env_reward = env_reward; a.term_flags = term_flags; a.drv_flags = drv_flags; a.route_feat = drv_route; a.route_info = drv_route_info;
    v.term_flags = term_flags; v.env_done = a.env_done; v.env_reward = env_reward; v.reset_mask = a.reset_mask; v.ep_length = a.ep_length;
    v.drv_flags = drv_flags; v.drv_info = drv_info; v.drv_feat = drv_feat; v.drv_route = drv_route; v.drv_route_info = drv_route_info;
    v.drv_progress = a.drv_progress; v.drv_reward = a.drv_reward; v.ep_return = a.ep_return; v.drv_done = a.drv_done;
    h->ep_state_bytes = state;
    h->ep_n = h->drivers.n;
    return SG_OK;
}

// sg_reset_scenarios / sg_reset_scenarios_device: the masked scenarios and their drivers start their accounting anew.  Without an
// episode in progress there is nothing to clear: the next tick zeroes everything.
int sgh::episode_clear_masked(sg_handle *h, const uint8_t *d_mask)
{
    if (!h->ep_live || h->drivers.n == 0 || h->ep_n != h->drivers.n) return SG_OK;
    sg::EpisodeArgs a = h->ep;
    a.R = h->R;
    a.n_drv = h->drivers.n;
    a.scen = h->drivers.scenarios();
    sgl::episode_clear(h->stream, d_mask, a);
    HIP_TRY(h, hipGetLastError());
    return SG_OK;
}

extern "C" int sg_tick_drivers(sg_handle *h, const double *actions, int32_t actions_device, const sg_episode_rules *rules, sg_episode_view *out)
{
    const char *who = "sg_tick_drivers";
    if (!h) return SG_ERR_INVALID;
    if (!rules || !out) return fail(h, SG_ERR_INVALID, "%s: null rules or out", who);
    if (!std::isfinite(rules->r_step) || !std::isfinite(rules->r_bad) || !std::isfinite(rules->w_progress))
        return fail(h, SG_ERR_INVALID, "%s: r_step, r_bad and w_progress must be finite", who);
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (h->drivers.n == 0) return fail(h, SG_ERR_STATE, "%s: no drivers set (sg_set_drivers)", who);
    if (const int rc = queue_gave_up(h)) return rc; // (sticky: nothing more is queued on a batch whose state is undefined)
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (const int rc = episode_layout(h)) return rc;
    if (!h->ep_live) // a new episode for everybody: no previous arclength, no return, no length
        HIP_TRY(h, hipMemsetAsync(h->episode.ptr, 0, h->ep_state_bytes, h->stream));
    h->ep_live = true;
    const bool progress = rules->w_progress != 0.0;
    const int32_t *d_scen = h->drivers.scenarios(), *d_slot = h->drivers.slots();
    // 1 - 3: the policy, the drivers' controllers, the step
    if (const int rc = drivers_step(h, 1, actions, actions_device, h->n_pol > 0, true)) return rc;
    // 4 - 6: what the rules read, of the stepped state
    const sg_episode_view &v = h->ep_view;
    sgl::terminal_flags(dim3((unsigned)h->R), h->stream, h->p, h->cfg.timestep, const_cast<uint32_t *>(v.term_flags));
    HIP_TRY(h, hipGetLastError());
    sgl::entity_status(h->stream, h->p, d_scen, d_slot, h->drivers.n, const_cast<uint32_t *>(v.drv_flags), const_cast<int32_t *>(v.drv_info),
                       const_cast<double *>(v.drv_feat));
    HIP_TRY(h, hipGetLastError());
    if (progress) {
        sgl::route_observation(h->stream, h->p, h->route, d_scen, d_slot, h->drivers.n, 0, 0.0, const_cast<double *>(v.drv_route),
                               const_cast<int32_t *>(v.drv_route_info));
        HIP_TRY(h, hipGetLastError());
    }
    // 7: reward, done, progress, statistics, the reset mask
    sg::EpisodeArgs a = h->ep;
    a.terminal_mask = rules->terminal_mask; a.bad_env_flags = rules->bad_env_flags; a.bad_driver_flags = rules->bad_driver_flags;
    a.auto_reset = rules->auto_reset;
    a.r_step = rules->r_step; a.r_bad = rules->r_bad; a.w_progress = rules->w_progress;
    a.R = h->R;
    a.n_drv = h->drivers.n;
    a.scen = d_scen;
    sgl::episode(h->stream, a);
    HIP_TRY(h, hipGetLastError());
    // 8: the scenarios that finished start anew (their accounting the kernel has zeroed itself)
    if (rules->auto_reset)
        if (const int rc = reset_scenarios_queued(h, v.reset_mask, false)) return rc;
    *out = v;
    if (!progress) {
        out->drv_route = nullptr;
        out->drv_route_info = nullptr;
    }
    return queue_gave_up(h); // (not waited for: what is known so far)
}
