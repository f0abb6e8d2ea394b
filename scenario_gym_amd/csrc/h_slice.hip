// h_slice.hip -- ScenarioGym.rollout time-sliced: the plan, whether it pays, the launches and their fix-ups.
#include "sgym_host.hpp"

using namespace sgh;

// ScenarioGym.rollout time-sliced (sgym_device.hpp, SliceArgs): the reset launch, the clock, the slices of the time axis
// side by side, the last executed step with the full state stores, the ordered sums.  For batches whose lanes are replay
// entities / replay agents -- and PID / vehicle agents: their controller pre-pass (control_kernel) then fills ONE table for
// the whole call, running ahead of the slices group by group.  Worth it when the batch alone cannot fill the chip (BASELINE
// config 2: 64 wavefronts; config 4's shards: 512); the results are bit-identical to launch_rollout's, the intermediate
// states are not written anywhere.
static void launch_slice_kernels(sg_handle *h, const Params &ps, const sg::SliceArgs &sa, dim3 grid, const double *tab)
{
    note_slice(h, tab != nullptr);
    sgl::rollout_slice(h->G, grid, h->stream, ps, h->cfg.timestep, sa, tab);
}
static void launch_fixup_kernel(sg_handle *h, const Params &ps, const sg::SliceArgs &sa)
{
    sgl::replay_fixup(h->G, dim3((unsigned)(h->NE / 64)), h->stream, ps, sa, h->d_n_final);
}

// slices, steps per slice and slices per launch group for a call of n_steps
struct SlicePlan { int S, len, SG; size_t bytes; };

static SlicePlan slice_plan(const sg_handle *h, int n_steps)
{
    const size_t nblk = h->NE / 64, R = (size_t)h->R, T1 = (size_t)n_steps + 1;
    const bool ctl = h->n_ctl > 0;
    SlicePlan pl{};
    // enough slices for ~4096 wavefronts per launch (mode 2, the tests' "always": short slices too)
    pl.SG = (int)std::max<size_t>(1, 4096 / nblk);
    if (ctl && h->slice_mode == 2) pl.SG = std::min(pl.SG, 8); // (the tests: several groups even for short calls)
    if (!ctl) { // one launch: all slices side by side, at least 64 steps each
        int S = (int)std::min<size_t>((size_t)pl.SG, (size_t)std::max(1, n_steps / (h->slice_mode == 2 ? 7 : 64)));
        pl.len = (n_steps + S - 1) / S;
        pl.S = (n_steps + pl.len - 1) / pl.len;
        pl.SG = pl.S;
    } else { // groups of SG slices of ~160 steps: a group starts when the pre-pass has passed its last step
        pl.len = std::min(n_steps, h->slice_mode == 2 ? 7 : std::max(16, env_int("SG_SLICE_LEN", 160)));
        pl.S = (n_steps + pl.len - 1) / pl.len;
    }
    // every array of the sliced path: |delta pose| rows, clocks, ego speeds, per-slice events and flags, and
    // the call-spanning controller table
    pl.bytes = nblk * T1 * 512 + h->clock_t0.size() * T1 * 8 + R * T1 * 16 +
               R * (size_t)pl.S * ((size_t)std::max(h->p.ev_cap, 1) * sizeof(sg_event) + 8) + R * 8 +
               (ctl ? (size_t)sg::CT_PLANES * sg::CT_W * (size_t)h->p.n_ctl_pad * T1 * 8 : 0);
    return pl;
}

bool sgh::slicing_pays(const sg_handle *h, int n_steps)
{
    if (!h->slice_mode || !h->sliceable || h->WV != 1 || h->p.rec_cap > 0 || h->rss_enabled || h->n_ext > 0 ||
        (h->cfg.terminal_mask & SG_TERM_EGO_OFF_ROAD) || n_steps < (h->slice_mode == 2 ? 2 : 512))
        return false;
    if (h->n_ctl > 0 && h->max_ctl_per_block > SG_TAB_LANES(h->G, h->WV)) return false; // (as launch_rollout's table path)
    const size_t nblk = h->NE / 64;
    if (nblk > 1024 && h->slice_mode != 2) return false; // more than one wavefront per SIMD: the batch fills the chip by itself
    return slice_plan(h, n_steps).bytes <= ((size_t)std::max(1, env_int("SG_SLICE_MB", 8192)) << 20);
}

int sgh::launch_sliced(sg_handle *h, int n_steps)
{
    const int R = h->R;
    const size_t nblk = h->NE / 64;
    const bool ctl = h->n_ctl > 0;
    const SlicePlan pl = slice_plan(h, n_steps);
    const int S = pl.S, len = pl.len;
    int rc;
    if (h->slice_T != n_steps || h->slice_S != S) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->ctl_stream));
        free_pool(h->slice_allocs);
        h->slice_T = -1;
        auto &A = h->slice_allocs;
        sg::SliceArgs sa{};
        double *tt = nullptr;
        const double *ct0 = nullptr;
        h->d_slice_tab = nullptr;
        rc = dev_alloc(h, A, &tt, (size_t)(n_steps + 1) * h->clock_t0.size(), false);
        sa.tt = tt;
        if (!rc) rc = dev_upload(h, A, &sa.clock_of, h->clock_of);
        if (!rc) rc = dev_upload(h, A, &ct0, h->clock_t0);
        h->d_clock_t0 = const_cast<double *>(ct0);
        if (!rc) rc = dev_alloc(h, A, &sa.dnorm, nblk * (size_t)(n_steps + 1) * 64, false);
        if (!rc) rc = dev_alloc(h, A, &sa.espeed, (size_t)R * (n_steps + 1), false);
        if (!rc) rc = dev_alloc(h, A, &sa.first_done, (size_t)R * S, false);
        if (!rc) rc = dev_alloc(h, A, &sa.ev, (size_t)R * S * std::max(h->p.ev_cap, 1), false);
        if (!rc) rc = dev_alloc(h, A, &sa.nev, (size_t)R * S, false);
        if (!rc) rc = dev_alloc(h, A, &h->d_n_final, (size_t)R, false);
        if (!rc) rc = dev_alloc(h, A, &h->d_slice_done, (size_t)R, false);
        if (!rc && ctl)
            rc = dev_alloc(h, A, &h->d_slice_tab, (size_t)sg::CT_PLANES * sg::CT_W * (size_t)h->p.n_ctl_pad * (size_t)(n_steps + 1), false);
        if (rc) { // out of device memory: not an error of the call -- the plain path needs none of these arrays
            (void)hipGetLastError();
            (void)hipStreamSynchronize(h->stream);
            free_pool(h->slice_allocs);
            h->err.clear();
            return SG_SLICE_FALLBACK;
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        sa.n_slices = S; sa.len = len; sa.n_total = n_steps;
        h->slice_args = sa;
        h->slice_T = n_steps;
        h->slice_S = S;
    }
    sg::SliceArgs sa = h->slice_args;
    Params ps = h->p;      // the kernels of this path address the controller table with the call's length
    ps.tab_steps = n_steps;
    const double *tab = ctl ? h->d_slice_tab : nullptr;
    h->n_launches = 0;
    h->launch_ev.clear();
    LaunchPlan reset = plan_call(h, 0, false, false); // State.reset by the batch's variant (not counted as a hot-path launch), timed
    reset.timed = true;
    size_t ev_next = 0;
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if ((rc = launch_main(h, reset, reset.reset_fam, 0, 1, 0, nullptr, nullptr, &ev_next))) return rc;
    hipEvent_t e_reset = nullptr;
    if (ctl) { // the pre-pass reads the reset state
        if ((rc = get_event(h, ev_next++, &e_reset))) return rc;
        HIP_TRY(h, hipEventRecord(e_reset, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(h->ctl_stream, e_reset, 0));
    }
    HIP_TRY(h, hipMemsetAsync(sa.first_done, 0x7f, (size_t)R * S * sizeof(int), h->stream)); // 0x7f7f7f7f: "never"
    HIP_TRY(h, hipMemsetAsync(sa.nev, 0, (size_t)R * S * sizeof(int), h->stream));
    const int n_clocks = (int)h->clock_t0.size();
    sgl::clock(dim3((unsigned)((n_clocks + 63) / 64)), h->stream, h->d_clock_t0, n_clocks, h->cfg.timestep, n_steps, const_cast<double *>(sa.tt));
    sa.mode = 0;
    const int ctl_len = std::max(1, env_int("SG_SLICE_CTL_STEPS", 2048)); // steps per control_kernel launch
    for (int s0 = 0; s0 < S; s0 += pl.SG) {
        const int ns = std::min(pl.SG, S - s0);
        if (ctl) { // rows (s0 * len, (s0 + ns) * len] of the table, then the event the group waits for
            const int k0 = s0 * len, k1 = std::min(n_steps, (s0 + ns) * len);
            const dim3 cgrid((unsigned)(ps.n_ctl_pad / 64));
            for (int k = k0; k < k1; k += ctl_len)
                sgl::control(sgl::CTL_FAST, cgrid, h->ctl_stream, ps, h->cfg.timestep, std::min(ctl_len, k1 - k), k == 0, k, nullptr, h->d_slice_tab, k, 0);
            HIP_TRY(h, hipGetLastError());
            hipEvent_t e_c = nullptr;
            if ((rc = get_event(h, ev_next++, &e_c))) return rc;
            HIP_TRY(h, hipEventRecord(e_c, h->ctl_stream));
            HIP_TRY(h, hipStreamWaitEvent(h->stream, e_c, 0));
        }
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if ((rc = get_event(h, ev_next, &e0)) || (rc = get_event(h, ev_next + 1, &e1))) return rc;
        HIP_TRY(h, hipEventRecord(e0, h->stream));
        sa.slice0 = s0;
        launch_slice_kernels(h, ps, sa, dim3((unsigned)nblk, (unsigned)ns), tab);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(e1, h->stream));
        h->launch_ev.push_back((int)ev_next);
        ++h->n_launches;
        ev_next += 2;
    }
    sa.slice0 = 0;
    sgl::slice_final(dim3((unsigned)((R + 63) / 64)), h->stream, ps, sa, h->d_n_final, h->d_slice_done);
    sa.mode = 1;
    sa.n_final = h->d_n_final;
    if (const int us = env_int("SG_SLICE_DELAY_US", 0)) sgl::delay(h->stream, (long long)us * 100ll); // 100 MHz
    launch_slice_kernels(h, ps, sa, dim3((unsigned)nblk, 1), tab);
    {   // the per-scenario ordered pass (a serial recurrence per scenario) on the second stream, beside the per-entity pass --
        // and AFTER the launch that materialises the last step: that launch starts from the scenario records of the reset
        // (clock, `done`, step count), which this pass overwrites with the final ones.  (Until round 5 it only waited for
        // slice_final_kernel and normally lost the race by a few microseconds; when it won -- seen on the first suite run of
        // cold boxes, one run in four -- a scenario it had already marked done sat the last launch out and kept its reset
        // poses.)
        hipEvent_t e_m1 = nullptr;
        if ((rc = get_event(h, ev_next++, &e_m1))) return rc;
        HIP_TRY(h, hipEventRecord(e_m1, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(h->ctl_stream, e_m1, 0));
        sgl::replay_scenario_fixup(dim3((unsigned)((R + 63) / 64)), h->ctl_stream, ps, sa, h->d_n_final, h->d_slice_done);
        if (ctl && h->p.ev_cap > 0) // the controlled egos' (and hazards') poses at the events: rows of the table
            sgl::event_ego_pose(dim3((unsigned)R), h->ctl_stream, ps, one_group(h, tab, n_steps));
    }
    launch_fixup_kernel(h, ps, sa);
    HIP_TRY(h, hipGetLastError());
    {
        hipEvent_t e_sc = nullptr;
        if ((rc = get_event(h, ev_next++, &e_sc))) return rc;
        HIP_TRY(h, hipEventRecord(e_sc, h->ctl_stream));
        HIP_TRY(h, hipStreamWaitEvent(h->stream, e_sc, 0));
    }
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return SG_OK;
}
