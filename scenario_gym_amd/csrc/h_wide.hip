// h_wide.hip -- scenarios of more than 512 entities: the multi-kernel step (sgym_wide.hpp).
#include "sgym_host.hpp"

using namespace sgh;

// Scenarios of more than 512 entities (sgym_wide.hpp): State.reset / n x ScenarioGym.step as four kernels per step.  Every
// scenario that may run steps in lockstep (a done scenario sits the step out unless `force`).  The host never waits here: every
// 64 steps a one-workgroup kernel writes the number of running scenarios into page-locked memory, and rollout() stops
// enqueuing once an EARLIER check point has answered 0 (what it enqueued in the meantime are no-ops).
constexpr unsigned WIDE_RING = 1024;
int sgh::ensure_wide(sg_handle *h) // (the scratch of the multi-kernel step; sg_tick calls it before it starts capturing)
{
    int rc = SG_OK;
    if (!h->wide_args.scr) {
        auto &A = h->wide_allocs;
        if ((rc = dev_alloc(h, A, &h->wide_args.scr, h->NE * sg::WS_W)) || (rc = dev_alloc(h, A, &h->wide_args.cor, h->NE * 8)) ||
            (rc = dev_alloc(h, A, &h->wide_args.circ, h->NE * 4)) || (rc = dev_alloc(h, A, &h->wide_args.last_row, (size_t)h->R * h->WV)) ||
            (rc = dev_alloc(h, A, &h->wide_args.last_same, h->NE)) || (rc = dev_alloc(h, A, &h->wide_args.dup, (size_t)h->R)) ||
            (rc = dev_alloc(h, A, &h->wide_args.walkers, (size_t)h->R)))
            return rc;
    }
    if (!h->wide_running) HIP_TRY(h, hipHostMalloc((void **)&h->wide_running, WIDE_RING * sizeof(int), hipHostMallocDefault));
    return SG_OK;
}

// (rss: sg_set_rss at this width -- RSSDistances.__call__ as a launch of its own after the reset and after every step)
int sgh::launch_wide(sg_handle *h, int n_steps, int do_reset, int force, const double *d_actions, bool rss)
{
    const int R = h->R, EP = h->EP;
    int rc = SG_OK;
    if ((rc = ensure_wide(h))) return rc;
    const dim3 ge((unsigned)((EP + 255) / 256), (unsigned)R), gs((unsigned)R);
    auto one = [&](int mode, const double *acts) {
        sg::WideArgs wa = h->wide_args;
        wa.mode = mode;
        wa.force = force;
        wa.actions = acts;
        wa.no_peds = h->has_ped ? 0 : 1;
        note_wide(h);
        sgl::wide_step(ge, gs, h->stream, h->p, h->cfg.timestep, wa, !h->has_ped);
    };
    if (do_reset) {
        one(do_reset == 2 ? 2 : 1, nullptr);
        if (rss) launch_rss_alone(h, do_reset == 2 ? 2 : 1);
        HIP_TRY(h, hipGetLastError());
    }
    const unsigned first_check = h->wide_check;
    for (int k = 0; k < n_steps; ++k) {
        one(0, d_actions ? d_actions + (size_t)k * R * 2 : nullptr);
        if (rss) launch_rss_alone(h, 0);
        if (!force && (k & 63) == 63 && k + 1 < n_steps) { // is anybody still running?
            HIP_TRY(h, hipGetLastError());
            bool nobody = false;
            for (unsigned c = first_check; c != h->wide_check && !nobody; ++c)
                nobody = __atomic_load_n(&h->wide_running[c % WIDE_RING], __ATOMIC_ACQUIRE) == 0;
            if (nobody) break;
            if (h->wide_check - first_check < WIDE_RING) { // (a call of more than 65,536 steps stops asking)
                int *word = &h->wide_running[h->wide_check++ % WIDE_RING];
                __atomic_store_n(word, -1, __ATOMIC_RELEASE);
                sgl::wide_running(h->stream, h->p, word);
            }
        }
    }
    HIP_TRY(h, hipGetLastError());
    return SG_OK;
}
