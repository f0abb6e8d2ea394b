// h_snapshot.hip -- device snapshots: one copy of every state array of a handle (sg_snapshot_create), the rows of the masked scenarios
// copied into it (sg_snapshot_save) or back (sg_snapshot_restore) by one launch of snapshot_copy_kernel (sgym_snapshot.hpp) on the
// handle's stream.  The state inventory -- what a later call can read of what an earlier call wrote -- is build_table() below, with
// kScratch beside it for what is left out and why; tests/test_snapshot_inventory.py holds the two against the arrays the handle owns.
#include "sgym_host.hpp"

using namespace sgh;

struct sg_snapshot {
    sg_handle *owner = nullptr;
    uint64_t upload_gen = 0, drivers_gen = 0; // of the handle when the snapshot was made
    bool rss_enabled = false, has_rss = false; // sg_set_rss then; the table holds the RSS records
    bool has_episode = false;                  // ... the episode accounting
    sg::SnapTable table{};
    char *buf = nullptr;                       // the one device allocation behind table.seg[..].snap
    uint64_t bytes = 0;
    uint8_t *d_mask = nullptr;                 // [R] where a HOST mask goes (stream-ordered: one buffer does)
    hipEvent_t join = nullptr;                 // the handle's controller stream joins its main stream through it
    // page-locked staging of HOST masks: a call takes a slot whose copy has run (or a new one) and never waits for the device
    struct Slot { uint8_t *host; hipEvent_t copied; };
    std::vector<Slot> slots;
};

namespace {

// Not state: every array a call writes before it reads it, so nothing an earlier call left there can reach a later call's results.
// (a list for readers and for the inventory test: no code reads it)
[[maybe_unused]] const char *const kScratch[][2] = {
    {"p.ctl_state", "scratch, because the pre-pass carries it from launch to launch of ONE call only: the first launch of every call takes the lane state from the blocks (control_body_l, `first`)"},
    {"p.phase_cycles", "scratch, because it is a profile counter of experiment builds (SG_PHASE_TIMERS) that no result reads"},
    {"wide_args.scr", "scratch, because wide_move_kernel writes every entity's row in the step that reads it"},
    {"wide_args.cor", "scratch, because wide_commit_kernel writes the corners of the step before the collision kernels read them"},
    {"wide_args.circ", "scratch, because wide_commit_kernel writes the circles of the step before the collision kernels read them"},
    {"wide_args.dup", "scratch, because wide_commit_kernel zeroes it every step before wide_collide_kernel raises it"},
    {"wide_args.walkers", "scratch, because wide_move_kernel counts the walkers of the step that advances noise_pos by them"},
    {"d_rssq", "scratch, because every launch fills the line-test queue before rss_lines_kernel drains it"},
    {"d_rssq_n", "scratch, because every launch writes the queue lengths before rss_lines_kernel reads them"},
    {"qwords", "scratch, because launch_queue resets the queue and progress words of every persistent launch"},
    {"d_qtab", "scratch, because the table ring is written by the pre-pass role of the launch that reads it"},
    {"d_tab", "scratch, because the controller tables are written by the pre-pass of the call that reads them"},
    {"slice_allocs", "scratch, because launch_sliced starts from a reset and fills its arrays itself"},
    {"sg_episode_view", "scratch, because the view arrays are outputs of the tick that wrote them: the next tick writes each before anybody reads it"},
};

struct TableBuilder {
    sg_handle *h;
    sg::SnapTable &t;
    uint64_t bytes = 0; // of the snapshot so far
    int rc = SG_OK;
    // One state array: `units` units of `unit` bytes per plane (SNAP_BLOCK: units = blocks, unit = 8).  Its place in the snapshot has
    // the live address modulo 16 and ends on a multiple of 16 with 16 bytes to spare, so no aligned word holds bytes of two arrays.
    void seg(const char *name, void *live, uint32_t kind, uint32_t unit, uint64_t units, uint32_t planes = 1, uint64_t plane_stride = 0,
             const int32_t *scen_of = nullptr, uint32_t rows = 0)
    {
        if (rc || !live || units == 0 || planes == 0) return;
        if (t.n == sg::SNAP_MAX_SEGS) { rc = fail(h, SG_ERR_INVALID, "sg_snapshot_create: no room in the segment table for %s", name); return; }
        sg::SnapSeg &s = t.seg[t.n++];
        s.live = static_cast<char *>(live);
        s.scen_of = scen_of;
        s.kind = kind; s.unit = unit; s.rows = rows; s.planes = planes;
        s.plane_bytes = kind == sg::SNAP_BLOCK ? units * rows * sg::ROW : units * unit;
        s.plane_stride = planes > 1 ? plane_stride : s.plane_bytes;
        s.chunks = (s.plane_bytes + 8 + 15) / 16; // (a plane may begin 8 bytes into its first chunk)
        assert(((uintptr_t)live & 7) == 0 && (planes == 1 || (s.plane_stride & 7) == 0));
        bytes = ((bytes + 15) & ~(uint64_t)15) + ((uintptr_t)live & 15);
        s.snap = reinterpret_cast<char *>(bytes); // (an offset until the buffer exists)
        bytes += (uint64_t)(planes - 1) * s.plane_stride + ((s.plane_bytes + 15) & ~(uint64_t)15) + 16;
    }
};

// The state inventory.  Every array here is read by some later call before that call writes it.
int build_table(sg_handle *h, sg_snapshot *s)
{
    const sg::Params &p = h->p;
    const uint64_t R = (uint64_t)h->R, EP = (uint64_t)h->EP, RE = R * EP;
    TableBuilder b{h, s->table};
    s->table.n = 0; s->table.R = h->R; s->table.EP = h->EP;
    // the batch (Upload::state_arrays)
    b.seg("p.dyn", p.dyn, sg::SNAP_BLOCK, 8, h->NE / 64, 1, 0, nullptr, (uint32_t)p.FROWS);
    b.seg("p.sdyn", p.sdyn, sg::SNAP_SCENARIO, (uint32_t)sizeof(sg_scenario_state), R);
    if (p.ev_cap > 0) {
        b.seg("p.events", p.events, sg::SNAP_SCENARIO, (uint32_t)(p.ev_cap * sizeof(sg_event)), R);
        b.seg("p.ev_pose", p.ev_pose, sg::SNAP_SCENARIO, (uint32_t)(p.ev_cap * 3 * sizeof(double)), R);
        b.seg("p.ev_hpose", p.ev_hpose, sg::SNAP_SCENARIO, (uint32_t)(p.ev_cap * 3 * sizeof(double)), R);
    }
    if (p.rec_cap > 0) { // the pose record: a plane [R] of times per row, a plane [R][EP] of one coordinate per row and coordinate
        b.seg("p.rec_t", p.rec_t, sg::SNAP_SCENARIO, 8, R, (uint32_t)p.rec_cap, R * 8);
        b.seg("p.rec_pose", p.rec_pose, sg::SNAP_ENTITY, 8, RE, (uint32_t)p.rec_cap * 6, RE * 8);
    }
    b.seg("h->d_ext", h->d_ext, sg::SNAP_ENTITY, 6 * sizeof(double), RE); // a caller-run slot keeps its pose until the caller sets another
    if (rss_live(h)) { // the RSSDistances records (h_rss.hip)
        b.seg("d_rss_state", h->d_rss_state, sg::SNAP_ENTITY, 4, RE);
        b.seg("d_rss_code", h->d_rss_code, sg::SNAP_ENTITY, 4, RE);
        b.seg("d_rss_safe", h->d_rss_safe, sg::SNAP_ENTITY, 2 * sizeof(double), RE);
        b.seg("d_rss_seen", h->d_rss_seen, sg::SNAP_SCENARIO, 4, R);
        s->has_rss = true;
    }
    if (h->wide) { // scenarios of more than 512 entities (h_wide.hip): CollisionMetric.last_timestep lives here, not in sg_scenario_state
        b.seg("wide_args.last_row", h->wide_args.last_row, sg::SNAP_SCENARIO, (uint32_t)(h->WV * 8), R);
        // (written by every step that runs; kept, because a scenario that sits a step out keeps what it had)
        b.seg("wide_args.last_same", h->wide_args.last_same, sg::SNAP_ENTITY, 4, RE);
    }
    if (h->drivers.n > 0) { // the episode accounting of sg_tick_drivers (the front of h->episode); a driver's row goes with its scenario
        const uint64_t n = (uint64_t)h->drivers.n;
        const int32_t *scen = h->drivers.scenarios();
        b.seg("prev_s", h->ep.prev_s, sg::SNAP_LIST, 8, n, 1, 0, scen);
        b.seg("acc_return", h->ep.acc_return, sg::SNAP_LIST, 8, n, 1, 0, scen);
        b.seg("acc_length", h->ep.acc_length, sg::SNAP_SCENARIO, 4, R);
        b.seg("prev_ok", h->ep.prev_ok, sg::SNAP_LIST, 1, n, 1, 0, scen);
        s->has_episode = true;
    }
    s->bytes = (b.bytes + 15) & ~(uint64_t)15;
    return b.rc;
}

// What every call on a snapshot checks before it queues anything.
int usable(sg_handle *h, const sg_snapshot *s, const char *who)
{
    if (!h) return SG_ERR_INVALID;
    if (!s) return fail(h, SG_ERR_INVALID, "%s: null snapshot", who);
    if (std::find(h->snapshots.begin(), h->snapshots.end(), s) == h->snapshots.end()) // (asked of the handle: s is not looked into)
        return fail(h, SG_ERR_INVALID, "%s: the snapshot belongs to another handle", who);
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (s->upload_gen != h->upload_gen)
        return fail(h, SG_ERR_STATE, "%s: the batch changed (sg_upload) since the snapshot was created: it can only be destroyed", who);
    if (s->drivers_gen != h->drivers_gen)
        return fail(h, SG_ERR_STATE, "%s: the driver list changed (sg_set_drivers) since the snapshot was created: it can only be destroyed", who);
    if (s->rss_enabled != h->rss_enabled || s->has_rss != rss_live(h))
        return fail(h, SG_ERR_STATE, "%s: sg_set_rss changed (or the RSS records came into being) since the snapshot was created: it can only be destroyed", who);
    return queue_gave_up(h); // (sticky: nothing more is queued on a batch whose state is undefined)
}

// A HOST mask on its way to s->d_mask through a page-locked slot; never waits for the device.
int stage_mask(sg_handle *h, sg_snapshot *s, const uint8_t *mask)
{
    sg_snapshot::Slot *slot = nullptr;
    for (auto &c : s->slots)
        if (hipEventQuery(c.copied) == hipSuccess) { slot = &c; break; }
    (void)hipGetLastError(); // (hipErrorNotReady of a slot whose copy is still queued)
    if (!slot) {
        sg_snapshot::Slot c{nullptr, nullptr};
        HIP_TRY(h, hipHostMalloc((void **)&c.host, (size_t)h->R, hipHostMallocDefault));
        if (hipEventCreateWithFlags(&c.copied, hipEventDisableTiming) != hipSuccess) {
            (void)hipHostFree(c.host);
            return fail(h, SG_ERR_HIP, "sg_snapshot: hipEventCreateWithFlags failed");
        }
        s->slots.push_back(c);
        slot = &s->slots.back();
    }
    memcpy(slot->host, mask, (size_t)h->R);
    HIP_TRY(h, hipMemcpyAsync(s->d_mask, slot->host, (size_t)h->R, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(slot->copied, h->stream));
    return SG_OK;
}

// save (restore == 0) or restore, queued on h->stream behind what either stream of the handle holds
int copy_queued(sg_handle *h, sg_snapshot *s, const uint8_t *mask, int32_t mask_device, int restore)
{
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // the controller stream joins the main stream, as the table path joins its pre-pass: an event there, a wait here, no host wait
    HIP_TRY(h, hipEventRecord(s->join, h->ctl_stream));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, s->join, 0));
    if (s->has_episode && !h->ep_live) { // the start-anew the next tick would do: the accounting of a fresh episode is zero
        HIP_TRY(h, hipMemsetAsync(h->episode.ptr, 0, h->ep_state_bytes, h->stream));
        h->ep_live = true;
    }
    const uint8_t *d_mask = nullptr;
    if (mask && mask_device) d_mask = mask;
    else if (mask) {
        if (const int rc = stage_mask(h, s, mask)) return rc;
        d_mask = s->d_mask;
    }
    if (!d_mask && h->snap_d2d) { // every scenario: one device-to-device copy per array
        for (int i = 0; i < s->table.n; ++i) {
            const sg::SnapSeg &g = s->table.seg[i];
            const size_t n = (size_t)(g.planes - 1) * g.plane_stride + g.plane_bytes;
            HIP_TRY(h, hipMemcpyAsync(restore ? g.live : g.snap, restore ? g.snap : g.live, n, hipMemcpyDeviceToDevice, h->stream));
        }
        return SG_OK;
    }
    sgl::snapshot_copy(h->stream, s->table, d_mask, restore);
    HIP_TRY(h, hipGetLastError());
    return SG_OK;
}

void release(sg_snapshot *s)
{
    if (s->buf) (void)hipFree(s->buf);
    if (s->d_mask) (void)hipFree(s->d_mask);
    if (s->join) (void)hipEventDestroy(s->join);
    for (auto &c : s->slots) {
        (void)hipEventDestroy(c.copied);
        (void)hipHostFree(c.host);
    }
    delete s;
}

} // namespace

void sgh::free_snapshots(sg_handle *h)
{
    for (sg_snapshot *s : h->snapshots) release(s);
    h->snapshots.clear();
}

extern "C" int sg_snapshot_create(sg_handle *h, sg_snapshot **out)
{
    const char *who = "sg_snapshot_create";
    if (!h) return SG_ERR_INVALID;
    if (!out) return fail(h, SG_ERR_INVALID, "%s: null out", who);
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "%s: no scenarios uploaded", who);
    if (const int rc = queue_gave_up(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // the arrays the handle makes on first use come into being now, as that use would make them
    if (h->rss_enabled && h->ego_first && !rss_live(h))
        if (const int rc = sg_rss_update(h, 1)) return rc;
    if (h->wide)
        if (const int rc = ensure_wide(h)) return rc;
    if (h->drivers.n > 0)
        if (const int rc = episode_layout(h)) return rc;
    std::unique_ptr<sg_snapshot, void (*)(sg_snapshot *)> s(new sg_snapshot, release);
    s->owner = h;
    s->upload_gen = h->upload_gen;
    s->drivers_gen = h->drivers_gen;
    s->rss_enabled = h->rss_enabled;
    if (const int rc = build_table(h, s.get())) return rc;
    HIP_TRY(h, hipMalloc((void **)&s->buf, (size_t)s->bytes));
    HIP_TRY(h, hipMalloc((void **)&s->d_mask, (size_t)h->R));
    HIP_TRY(h, hipEventCreateWithFlags(&s->join, hipEventDisableTiming));
    for (int i = 0; i < s->table.n; ++i) s->table.seg[i].snap = s->buf + reinterpret_cast<uintptr_t>(s->table.seg[i].snap);
    HIP_TRY(h, hipMemsetAsync(s->buf, 0, (size_t)s->bytes, h->stream)); // (the padding between the arrays is never read as state)
    if (const int rc = copy_queued(h, s.get(), nullptr, 0, 0)) return rc; // every scenario: no row of a snapshot is ever unsaved
    h->snapshots.push_back(s.get());
    *out = s.release();
    return SG_OK;
}

extern "C" int sg_snapshot_save(sg_handle *h, sg_snapshot *s, const uint8_t *mask, int32_t mask_device)
{
    if (const int rc = usable(h, s, "sg_snapshot_save")) return rc;
    return copy_queued(h, s, mask, mask_device, 0);
}

extern "C" int sg_snapshot_restore(sg_handle *h, sg_snapshot *s, const uint8_t *mask, int32_t mask_device)
{
    if (const int rc = usable(h, s, "sg_snapshot_restore")) return rc;
    return copy_queued(h, s, mask, mask_device, 1);
}

extern "C" int sg_snapshot_bytes(sg_handle *h, const sg_snapshot *s, uint64_t *bytes)
{
    if (!h) return SG_ERR_INVALID;
    if (!s || !bytes) return fail(h, SG_ERR_INVALID, "sg_snapshot_bytes: null snapshot or bytes");
    if (std::find(h->snapshots.begin(), h->snapshots.end(), s) == h->snapshots.end())
        return fail(h, SG_ERR_INVALID, "sg_snapshot_bytes: the snapshot belongs to another handle");
    *bytes = s->bytes;
    return SG_OK;
}

extern "C" int sg_snapshot_destroy(sg_handle *h, sg_snapshot *s)
{
    if (!h) return SG_ERR_INVALID;
    if (!s) return fail(h, SG_ERR_INVALID, "sg_snapshot_destroy: null snapshot");
    const auto it = std::find(h->snapshots.begin(), h->snapshots.end(), s);
    if (it == h->snapshots.end()) return fail(h, SG_ERR_INVALID, "sg_snapshot_destroy: the snapshot belongs to another handle");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (a queued save or restore may still use it)
    h->snapshots.erase(it);
    release(s);
    return SG_OK;
}
