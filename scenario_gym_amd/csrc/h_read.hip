// h_read.hip -- reading results back: the state view, the metrics and events, collision points, the recorded poses.
#include "sgym_host.hpp"

using namespace sgh;

extern "C" int sg_state_view_get(sg_handle *h, sg_state_view *out)
{
    if (!h || !out) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_state_view_get: no scenarios uploaded");
    out->n_scenarios = h->R; out->n_entities = h->E; out->entity_stride = h->EP;
    out->n_blocks = (int32_t)(h->NE / 64);
    out->row_words = h->WV;
    out->block_rows = h->p.FROWS;
    out->blocks = h->p.dyn;
    out->scen = h->p.sdyn;
    return SG_OK;
}

extern "C" int sg_read_metrics(sg_handle *h, sg_metrics *out, sg_event *events, int32_t cap, int32_t *n_events)
{
    if (!h || !out) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_read_metrics: no scenarios uploaded");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (events && h->p.ev_cap > 0) { // CollisionMetric.record_collision for the Vehicle hazards recorded since the last read
        sgl::classify_events(dim3((unsigned)h->R), h->stream, h->p, h->c_tol);
        HIP_TRY(h, hipGetLastError());
    }
    const int R = h->R;
    const Params &p = h->p;
    int rc0 = h->pin_sd.ensure(h, (size_t)R * sizeof(sg_scenario_state)); // (page-locked, grown on demand, kept on the handle)
    if (rc0) return rc0;
    sg_scenario_state *sd = h->pin_sd.as<sg_scenario_state>();
    HIP_TRY(h, hipMemcpyAsync(sd, p.sdyn, (size_t)R * sizeof(sg_scenario_state), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if ((rc0 = check_queue(h))) return rc0;
    int64_t total = 0;
    bool overflow = false;
    for (int r = 0; r < R; ++r) {
        out[r].ego_avg_speed = sd[r].ego_avg_speed; out[r].ego_max_speed = sd[r].ego_max_speed;
        out[r].ego_distance_travelled = sd[r].ego_distance_travelled;
        out[r].final_t = sd[r].t; out[r].n_steps = sd[r].n_steps; out[r].done = sd[r].done;
        out[r].n_collisions = sd[r].n_events;
        out[r].reserved = 0;
        if (h->noise_mode == SG_NOISE_STREAM && h->has_ped && sd[r].noise_pos > h->noise_len)
            return fail(h, SG_ERR_CAPACITY, "sg_read_metrics: scenario %d needed %lld noise variates, the stream of sg_set_ped_noise holds %lld",
                        r, (long long)sd[r].noise_pos, (long long)h->noise_len);
        if (sd[r].n_events > p.ev_cap) overflow = true;
        total += std::min(sd[r].n_events, p.ev_cap);
    }
    if (n_events) *n_events = (int32_t)total;
    if (events && cap > 0 && p.ev_cap > 0 && total > 0) {
        int width = 0; // only the columns in use travel over PCIe
        for (int r = 0; r < R; ++r) width = std::max(width, std::min(sd[r].n_events, p.ev_cap));
        if ((rc0 = h->pin_ev.ensure(h, (size_t)R * width * sizeof(sg_event)))) return rc0;
        sg_event *all = h->pin_ev.as<sg_event>();
        HIP_TRY(h, hipMemcpy2DAsync(all, (size_t)width * sizeof(sg_event), p.events, (size_t)p.ev_cap * sizeof(sg_event),
                                    (size_t)width * sizeof(sg_event), (size_t)R, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        int64_t k = 0;
        for (int r = 0; r < R; ++r)
            for (int i = 0; i < std::min(sd[r].n_events, p.ev_cap); ++i) {
                if (k >= cap) return fail(h, SG_ERR_CAPACITY, "sg_read_metrics: %lld events do not fit cap=%d", (long long)total, cap);
                events[k++] = all[(size_t)r * width + i];
            }
    }
    // more than event_capacity events in one scenario: the count (n_collisions) is exact, the table keeps the first ones
    (void)overflow;
    return SG_OK;
}

// CollisionPointMetric.get_state (metrics/collision.py:217-253) for the events sg_read_metrics lists, in its order
extern "C" int sg_read_collision_points(sg_handle *h, double *out, int32_t cap, int32_t *n_events)
{
    if (!h || !out) return h ? fail(h, SG_ERR_INVALID, "sg_read_collision_points: null argument") : SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_read_collision_points: no scenarios uploaded");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int R = h->R;
    const Params &p = h->p;
    if (p.ev_cap > 0) {
        sgl::classify_events(dim3((unsigned)R), h->stream, p, h->c_tol);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (const int rcq = check_queue(h)) return rcq; // (a persistent launch that gave up: sticky)
    std::vector<sg_scenario_state> sd(R);
    HIP_TRY(h, hipMemcpy(sd.data(), p.sdyn, (size_t)R * sizeof(sg_scenario_state), hipMemcpyDeviceToHost));
    std::vector<double> all((size_t)R * std::max(p.ev_cap, 1) * 3);
    HIP_TRY(h, hipMemcpy(all.data(), p.ev_pose, all.size() * sizeof(double), hipMemcpyDeviceToHost));
    int64_t k = 0;
    for (int r = 0; r < R; ++r)
        for (int i = 0; i < std::min(sd[r].n_events, p.ev_cap); ++i, ++k) {
            if (k >= cap) return fail(h, SG_ERR_CAPACITY, "sg_read_collision_points: more events than cap=%d", cap);
            for (int c = 0; c < 3; ++c) out[k * 3 + c] = all[((size_t)r * p.ev_cap + i) * 3 + c];
        }
    if (n_events) *n_events = (int32_t)k;
    return SG_OK;
}

extern "C" int sg_read_record(sg_handle *h, int32_t n_rows, double *t_out, double *pose_out)
{
    if (!h || n_rows < 0) return SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_read_record: no scenarios uploaded");
    const Params &p = h->p;
    if (n_rows > p.rec_cap) return fail(h, SG_ERR_CAPACITY, "sg_read_record: n_rows=%d > record_capacity=%d", n_rows, p.rec_cap);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (const int rcq = check_queue(h)) return rcq; // (a persistent launch that gave up: sticky)
    const int R = h->R, E = h->E, EP = h->EP;
    if (t_out && n_rows) HIP_TRY(h, hipMemcpy(t_out, p.rec_t, (size_t)n_rows * R * 8, hipMemcpyDeviceToHost));
    if (pose_out && n_rows) {
        std::vector<double> raw((size_t)n_rows * 6 * R * EP);
        HIP_TRY(h, hipMemcpy(raw.data(), p.rec_pose, raw.size() * 8, hipMemcpyDeviceToHost));
        for (int s = 0; s < n_rows; ++s)
            for (int r = 0; r < R; ++r)
                for (int e = 0; e < E; ++e)
                    for (int c = 0; c < 6; ++c)
                        pose_out[(((size_t)s * R + r) * E + e) * 6 + c] = raw[((size_t)s * 6 + c) * R * EP + (size_t)r * EP + e];
    }
    return SG_OK;
}
