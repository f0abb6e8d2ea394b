// sgym_hip.hip -- the dispatcher of libsgym_hip.so: which rollout kernel family and which schedule a call of the C ABI
// (include/sgym.h) takes, and the stepping entry points.  The rest of the host side: h_*.hip around sgym_host.hpp.
#include "sgym_host.hpp"

using namespace sgh;

// the entry point the handle launched last for a step loop (sg_last_kernel): what a kernel trace of the call shows
static void note_kernel(sg_handle *h, const char *fmt, int a = 0, int b = 0) { snprintf(h->last_kernel, sizeof h->last_kernel, fmt, a, b); }
// (every note_kernel call is in this file -- tests/test_gpu_variants.py reads the names here: the schedules of other units say
// theirs through these)
void sgh::note_wide(sg_handle *h) { note_kernel(h, "sg::wide_move_kernel + wide_commit_kernel + wide_collide_kernel + wide_finish_kernel"); }
void sgh::note_queue(sg_handle *h, bool rss)
{
    note_kernel(h, rss ? "sg::rollout_kernel_rss_tabq<%d>" : (h->planar ? "sg::rollout_kernel_tabq_planar<%d>" : "sg::rollout_kernel_tabq<%d>"), h->G);
}
void sgh::note_slice(sg_handle *h, bool tab) { note_kernel(h, tab ? "sg::rollout_kernel_slice_tab<%d>" : "sg::rollout_kernel_slice<%d>", h->G); }

// the family of a launch for this handle's batch: `rss` the RSS callback inside the kernel (it fills the line-test queue),
// `tab` the controlled lanes' poses from the pre-pass table (plan_call)
static Fam pick_family(const sg_handle *h, bool rss, bool tab)
{
    const bool ped = h->has_ped, off_road = (h->cfg.terminal_mask & SG_TERM_EGO_OFF_ROAD) != 0;
    if (h->WV == 8) { // 257..512 entities (the table path never runs at this width)
        if (!ped && off_road) return Fam::ROAD_W8;
        if (rss && !ped) return Fam::RSS_W8;
        return ped ? Fam::PED_W8 : Fam::PLAIN_W8;
    }
    if (ped && h->all_ped && h->G == 64 && crowd_road_ok(h) && crowd_allowed(h) && !rss) return Fam::CROWD;
    if (tab && ped && h->G == 64) return Fam::CROWD_RIDERS;
    if (ped && rss) return Fam::RSS_PED;
    if (rss && off_road) return Fam::RSS_ROAD;
    if (ped) return Fam::PED;
    if (rss && tab && h->WV == 1) return Fam::RSS_TAB;
    if (rss) return Fam::RSS;
    if (off_road) return Fam::ROAD;
    if (tab && h->WV == 1 && h->n_ctl > 0) return Fam::TAB;
    return tab ? Fam::TAB_ROWS : Fam::PLAIN;
}

static void launch_variant(sg_handle *h, Fam fam, dim3 grid, int n_steps, int do_reset, int force, const double *d_actions,
                           const double *d_tab, const sg::TabGroups &tg)
{
    const int G = h->G, WV = h->WV;
    const hipStream_t s = h->stream;
    const sgl::RolloutArgs a{&h->p, h->cfg.timestep, n_steps, do_reset, force, d_actions, nullptr};
    const sgl::RolloutArgs at{&h->p, h->cfg.timestep, n_steps, 0, force, nullptr, d_tab}; // table variants never reset
    switch (fam) {
    // 257..512 entities, eight wavefronts: ego_off_road / the RSS callback inside / pedestrian agents / vehicles and replay only
    case Fam::ROAD_W8: note_kernel(h, "sg::rollout_kernel_road<64, 8>"); sgl::rollout_road(64, 8, grid, s, a); break;
    case Fam::RSS_W8: note_kernel(h, "sg::rollout_kernel_rss<64, 8>"); sgl::rollout_rss(64, 8, false, grid, s, a); break;
    case Fam::PED_W8: note_kernel(h, "sg::rollout_kernel<64, 8, true, false>"); sgl::rollout_ped(64, 8, false, grid, s, a); break;
    case Fam::PLAIN_W8: note_kernel(h, "sg::rollout_kernel<64, 8, false, false>"); sgl::rollout_plain(64, 8, false, grid, s, a); break;
    case Fam::CROWD: note_kernel(h, h->n_ped_models > 1 ? "sg::rollout_kernel_crowd_models<%d>" : "sg::rollout_kernel_crowd<%d>", WV);
        sgl::rollout_crowd(WV, false, grid, s, a, h->n_ped_models > 1); break;
    case Fam::CROWD_RIDERS: note_kernel(h, "sg::rollout_kernel_crowd_riders<%d>", WV); sgl::rollout_crowd(WV, true, grid, s, at); break;
    case Fam::RSS_PED: note_kernel(h, "sg::rollout_kernel_rss_ped<%d, %d>", std::max(G, 16), WV); sgl::rollout_ped(G, WV, true, grid, s, a); break;
    case Fam::RSS_ROAD: note_kernel(h, "sg::rollout_kernel_rss_road<%d, %d>", G, WV); sgl::rollout_rss(G, WV, true, grid, s, a); break;
    case Fam::PED: note_kernel(h, "sg::rollout_kernel<%d, %d, true, false>", std::max(G, 16), WV); sgl::rollout_ped(G, WV, false, grid, s, a); break;
    case Fam::RSS_TAB: note_kernel(h, "sg::rollout_kernel_rss_tab<%d>", G); sgl::rollout_rss_tab(G, tab_grid(h, tg), s, h->p, h->cfg.timestep, force, tg); break;
    case Fam::RSS: note_kernel(h, "sg::rollout_kernel_rss<%d, %d>", G, WV); sgl::rollout_rss(G, WV, false, grid, s, a); break;
    case Fam::ROAD: note_kernel(h, "sg::rollout_kernel_road<%d, %d>", G, WV); sgl::rollout_road(G, WV, grid, s, a); break;
    case Fam::TAB: note_kernel(h, h->planar ? "sg::rollout_kernel_tab_planar<%d>" : "sg::rollout_kernel_tab<%d>", G);
        sgl::rollout_tab(G, h->planar, tab_grid(h, tg), s, h->p, h->cfg.timestep, force, tg); break;
    case Fam::TAB_ROWS: note_kernel(h, "sg::rollout_kernel<%d, %d, false, true>", G, WV); sgl::rollout_plain(G, WV, true, grid, s, at); break;
    case Fam::PLAIN: note_kernel(h, "sg::rollout_kernel<%d, %d, false, false>", G, WV); sgl::rollout_plain(G, WV, false, grid, s, a); break;
    }
}

int sgh::get_event(sg_handle *h, size_t idx, hipEvent_t *out)
{
    while (h->ev_pool.size() <= idx) {
        hipEvent_t e;
        HIP_TRY(h, hipEventCreate(&e));
        h->ev_pool.push_back(e);
    }
    *out = h->ev_pool[idx];
    return SG_OK;
}

// one rollout_kernel launch of family `fam` on the handle's stream, bracketed by its own pair of timing events when the plan is
// timed (d_tab: a table variant's table; groups: the block groups of a grouped table-variant launch, else every block runs n_steps)
int sgh::launch_main(sg_handle *h, const LaunchPlan &pl, Fam fam, int n_steps, int do_reset, int force, const double *d_actions,
                     const double *d_tab, size_t *ev_next, const sg::TabGroups *groups)
{
    const sg::TabGroups tg = groups ? *groups : one_group(h, d_tab, n_steps);
    dim3 grid(h->WV == 1 ? (unsigned)(h->NE / 64) : (unsigned)h->R);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc;
    if (pl.timed) {
        if ((rc = get_event(h, *ev_next, &e0)) || (rc = get_event(h, *ev_next + 1, &e1))) return rc;
        HIP_TRY(h, hipEventRecord(e0, h->stream));
    }
    launch_variant(h, fam, grid, n_steps, do_reset, force, d_actions, d_tab, tg);
    HIP_TRY(h, hipGetLastError());
    if (d_tab && h->n_ctl > 0 && h->p.ev_cap > 0 && n_steps > 0) {
        // a controlled ego's pose at an event of this chunk is a row of the chunk's controller table: copied into the event
        // now -- before the event below, which the pre-pass of a later chunk waits for before it reuses the buffer
        sgl::event_ego_pose(dim3((unsigned)h->R), h->stream, h->p, tg);
        HIP_TRY(h, hipGetLastError());
    }
    if (pl.rss_lines) { // (launch_variant ran a rollout_kernel_rss* variant)
        sgl::rss_lines(tab_grid(h, tg), h->stream, h->p, tg);
        HIP_TRY(h, hipGetLastError());
    }
    if (!pl.timed) return SG_OK;
    HIP_TRY(h, hipEventRecord(e1, h->stream));
    if (n_steps > 0) { // reset-only launches are not counted as hot-path launches
        h->launch_ev.push_back((int)*ev_next);
        ++h->n_launches;
    }
    *ev_next += 2;
    return SG_OK;
}

// the ego_off_road terminal condition behind a step of a variant without it (plan_call's off_road)
static void launch_off_road(sg_handle *h) { sgl::ego_off_road(dim3((unsigned)((h->R + 63) / 64)), h->stream, h->p); }

// What a call of n_steps steps launches (`rss`: the RSS callback runs inside the rollout kernel, rss_fused_call; `allow_tab`: the
// table path may be taken).  Pure: no HIP calls, nothing written; the environment is read per call.
LaunchPlan sgh::plan_call(const sg_handle *h, int n_steps, bool rss, bool allow_tab)
{
    LaunchPlan pl;
    const bool off_road = (h->cfg.terminal_mask & SG_TERM_EGO_OFF_ROAD) != 0;
    if (h->wide) { // RSSDistances.__call__ as a launch of its own after the reset and after every step; timed from 16 steps
        pl.schedule = SCHED_WIDE;
        pl.rss_alone = rss;
        pl.timed = n_steps >= 16;
        return pl;
    }
    // Combinations no fused variant carries go step by step with the missing part as a launch of its own behind every step:
    // pedestrian agents AND the ego_off_road terminal condition (ego_off_road_kernel: check_terminal is the last thing a step
    // does to `done`, so a condition added afterwards is the same as one in the list); the RSS callback on scenarios of
    // 257..512 entities with pedestrian agents or ego_off_road (rss_kernel, as beyond 512).  A scenario that is done sits
    // the later launches out.  Rare enough combinations not to deserve kernel variants of their own.  Not timed.
    pl.off_road = h->has_ped && off_road;
    pl.rss_alone = rss && h->WV == 8 && (h->has_ped || off_road);
    pl.rss_lines = rss && !pl.rss_alone;
    if (pl.off_road || pl.rss_alone) {
        pl.schedule = SCHED_STEPWISE;
        pl.reset_fam = pl.fam = pick_family(h, pl.rss_lines, false);
        return pl;
    }
    // the table variant serves SG_TAB_LANES controlled lanes per wavefront; denser batches keep their controllers
    // in the rollout kernel, where they fill the wavefront anyway
    // (a crowd with riders: lanes of other kinds ride the crowd kernel on a pre-pass table; short calls -- the per-tick loop of
    // an RL driver -- keep the general pedestrian variant, like the table path keeps the in-kernel controllers)
    pl.riders = allow_tab && h->crowd_riders && crowd_road_ok(h) && !rss && h->n_ctl > 0 && n_steps >= h->tab_min;
    // (the RSS callback inside the kernel: its controlled lanes ride the table too -- rollout_kernel_rss_tab -- which takes the
    // controller code out of the one variant that has no issue slot to spare; launches stay within the line-test queue)
    pl.rss_tab = allow_tab && rss && h->WV == 1 && !h->has_ped && !off_road && h->n_ext == 0 && h->n_ctl > 0 && n_steps >= h->tab_min &&
                 env_int("SG_RSS_TAB", 1) != 0;
    const bool use_tab = pl.riders || pl.rss_tab || (allow_tab && h->WV <= 4 && !h->has_ped && !rss && !off_road && h->n_ext == 0 &&
                                                     n_steps >= h->tab_min && h->max_ctl_per_block <= SG_TAB_LANES(h->G, h->WV));
    // short calls (the per-tick loop of an RL driver) are not timed: four event records cost more than their kernel
    pl.timed = use_tab || n_steps >= 16;
    pl.reset_fam = pick_family(h, rss, false);
    pl.fam = pick_family(h, rss, use_tab);
    pl.schedule = !use_tab ? SCHED_ONE : h->n_ctl == 0 ? SCHED_TAB_DUMMY : SCHED_TAB;
    // the table path's pre-pass: the riders' own; the fast one for the RSS table variant (the ego's metrics are the rollout
    // kernel's, from its own velocities); else the general one, which keeps the ego's metrics
    if (pl.riders) pl.ctl = sgl::CTL_RIDERS;
    else if (pl.rss_tab && env_int("SG_RSS_CTL_FAST", 1) != 0) pl.ctl = sgl::CTL_FAST;
    pl.ctl_metrics = pl.riders || pl.rss_tab ? 0 : 1;
    return pl;
}

// ScenarioGym.rollout / n x step for the whole batch as `pl` says (every schedule but the time-sliced one).  Scenarios without
// pedestrians and with at least SG_TAB_MIN_STEPS steps to do take the two-kernel path: control_kernel integrates the PID / vehicle
// agents for a chunk of steps on its own stream while rollout_kernel<TAB> consumes the previous chunks' tables.  Only the table
// path synchronises (to grow a buffer): sg_tick, which never takes it, runs this inside its graph capture.
int sgh::launch_plan(sg_handle *h, const LaunchPlan &pl, int n_steps, int do_reset, int force, const double *d_actions)
{
    h->n_launches = 0;
    h->launch_ev.clear();
    if (pl.timed) HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    size_t ev_next = 0;
    int rc = SG_OK;
    switch (pl.schedule) {
    case SCHED_WIDE: // scenarios of more than 512 entities: the multi-kernel step
        rc = launch_wide(h, n_steps, do_reset, force, d_actions, pl.rss_alone);
        break;
    case SCHED_STEPWISE: // one launch per step, each followed by what no fused variant carries (rss_alone, off_road)
        h->timed = false;
        if (do_reset && !(rc = launch_main(h, pl, pl.reset_fam, 0, do_reset, 0, nullptr, nullptr, &ev_next)) && pl.rss_alone)
            launch_rss_alone(h, do_reset == 2 ? 2 : 1);
        for (int k = 0; k < n_steps && !rc; ++k) {
            if ((rc = launch_main(h, pl, pl.fam, 1, 0, force, d_actions ? d_actions + (size_t)k * h->R * 2 : nullptr, nullptr, &ev_next))) break;
            if (pl.off_road) launch_off_road(h);
            if (pl.rss_alone) launch_rss_alone(h, 0);
        }
        if (!rc) HIP_TRY(h, hipGetLastError());
        break;
    case SCHED_ONE: { // one launch for the reset and every step (launches of rssq_steps steps when they fill the line-test queue)
        const int per = pl.rss_lines ? std::max(1, h->rssq_steps) : n_steps;
        int k0 = 0;
        do {
            rc = launch_main(h, pl, pl.fam, std::min(per, n_steps - k0), k0 == 0 ? do_reset : 0, force,
                             d_actions ? d_actions + (size_t)k0 * h->R * 2 : nullptr, nullptr, &ev_next);
        } while (!rc && (k0 += per) < n_steps);
        break;
    }
    case SCHED_TAB_DUMMY:
    case SCHED_TAB: // the table path (table variants never reset: the reset is a launch of the non-table variant)
        if (!do_reset || !(rc = launch_main(h, pl, pl.reset_fam, 0, do_reset, 0, nullptr, nullptr, &ev_next)))
            rc = launch_table(h, pl, n_steps, force, d_actions, &ev_next);
        break;
    }
    if (rc) return rc;
    if (pl.timed) HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    h->timed = pl.timed;
    return SG_OK;
}

// a call of the C ABI: plan, launch, and after a failure wait for what is still running
int sgh::launch_rollout(sg_handle *h, int n_steps, int do_reset, int force, const double *d_actions, bool rss)
{
    if (do_reset == 1) forget_queue_failure(h); // (State.reset of the whole batch: until then a give-up is sticky)
    int rc = h->q_failed ? fail(h, SG_ERR_HIP, "%s", h->q_msg) : SG_OK;
    if (!rc) {
        h->last_schedule = 0;
        rc = launch_plan(h, plan_call(h, n_steps, rss, true), n_steps, do_reset, force, d_actions);
    }
    if (rc) drain_streams(h);
    return rc;
}

// Does this call hand the RSS callback to its launches (plan_call: inside the rollout kernel, or rss_kernel behind every step)?
// sg_set_rss on, the ego entity 0 of every scenario, and for `live_only` callers records of this batch from an earlier call.
// Then the records and the line-test queue are made here, before any graph capture (sg_tick); *fresh: the records are new.
int sgh::rss_fused_call(sg_handle *h, bool live_only, bool *fused, bool *fresh)
{
    bool made = false;
    int rc = SG_OK;
    *fused = h->rss_enabled && h->ego_first && (!live_only || rss_live(h));
    if (*fused && !(rc = ensure_rss(h, &made))) rc = ensure_rssq(h);
    if (fresh) *fresh = made;
    return rc;
}

// room for n doubles of actions (n is 0 or at least R * 2); callers that hand the address to a graph bump `generation` on *grew
int sgh::ensure_actions(sg_handle *h, size_t n, bool *grew) { return h->actions.ensure(h, n * sizeof(double), grew); }

// the stepping of sg_step, and of every step of sg_step_drivers (h_drive.hip): forced steps, the RSS callback as the handle has it
int sgh::step_forced(sg_handle *h, int n_steps, const double *d_act)
{
    bool fused = false;
    int rc = rss_fused_call(h, true, &fused);
    if (rc) return rc;
    if (h->rss_enabled && !fused) { // (no records of this batch yet, or the ego is not entity 0) one step per launch
        for (int k = 0; k < n_steps && !rc; ++k)
            if (!(rc = launch_rollout(h, 1, 0, 1, d_act + (size_t)k * h->R * 2))) rc = sg_rss_update(h, 0);
    } else {
        rc = launch_rollout(h, n_steps, 0, 1, d_act, fused);
    }
    return rc;
}

extern "C" int sg_step(sg_handle *h, int32_t n_steps, const double *actions, int32_t actions_device)
{
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_step: no scenarios uploaded");
    if (n_steps < 0) return fail(h, SG_ERR_INVALID, "sg_step: n_steps < 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const double *d_act = nullptr;
    if (actions && actions_device) {
        d_act = actions;
    } else if (actions) {
        size_t n = (size_t)n_steps * h->R * 2;
        if (int rc0 = ensure_actions(h, n)) return rc0;
        if (n) HIP_TRY(h, hipMemcpyAsync(h->actions.ptr, actions, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        d_act = h->actions.as<double>();
    } else {
        // no actions: SG_KIND_AGENT_VEHICLE slots get (0, 0)
        size_t n = (size_t)n_steps * h->R * 2;
        if (int rc0 = ensure_actions(h, n)) return rc0;
        if (n) HIP_TRY(h, hipMemsetAsync(h->actions.ptr, 0, n * sizeof(double), h->stream));
        d_act = h->actions.as<double>();
    }
    if (const int rc = step_forced(h, n_steps, d_act)) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return check_queue(h);
}

extern "C" int sg_rollout_async(sg_handle *h, int32_t max_steps, int32_t do_reset)
{
    if (!h) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_rollout: no scenarios uploaded");
    if (h->n_ext > 0 && max_steps > 0)
        return fail(h, SG_ERR_STATE, "sg_rollout: %d slots are driven by the caller's agents (SG_KIND_AGENT_EXTERNAL): "
                                     "use sg_set_external_poses + sg_step tick by tick", h->n_ext);
    if (max_steps < 0) return fail(h, SG_ERR_INVALID, "sg_rollout: max_steps < 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // the callback inside the rollout kernel (rollout_kernel_rss): after the reset and after every step of ONE launch
    bool fused = false, fresh = false;
    int rc = rss_fused_call(h, false, &fused, &fresh);
    if (rc) return rc;
    if (fused) return launch_rollout(h, max_steps, do_reset || fresh ? 1 : 0, 0, nullptr, true);
    if (h->rss_enabled) { // (sg_rss_update reports why not: the ego is not entity 0) one step per launch
        if (do_reset && ((rc = launch_rollout(h, 0, 1, 0, nullptr)) || (rc = sg_rss_update(h, 1)))) return rc;
        for (int k = 0; k < max_steps; ++k)
            if ((rc = launch_rollout(h, 1, 0, 0, nullptr)) || (rc = sg_rss_update(h, 0))) return rc;
        return SG_OK;
    }
    if (do_reset && slicing_pays(h, max_steps)) {
        rc = launch_sliced(h, max_steps);
        if (rc != SG_SLICE_FALLBACK) return rc;
    }
    // external-action slots are fed (0, 0) here; drive them with sg_step(actions)
    return launch_rollout(h, max_steps, do_reset ? 1 : 0, 0, nullptr);
}

extern "C" int sg_rollout(sg_handle *h, int32_t max_steps)
{
    int rc = sg_rollout_async(h, max_steps, 1);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return check_queue(h);
}

extern "C" int sg_synchronize(sg_handle *h)
{
    if (!h) return SG_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return check_queue(h);
}
