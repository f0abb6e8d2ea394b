// h_queue.hip -- the table path: the persistent queue launch (sgym_queue.hpp), its give-up bookkeeping, the chunk launches.
#include "sgym_host.hpp"

using namespace sgh;

enum { Q_HOST_RING = 16 };
// after a synchronisation of h->stream: did every persistent launch since the last look run to its end?  (Sticky: see q_failed.)
int sgh::check_queue(sg_handle *h)
{
    for (; h->q_count > 0; --h->q_count) {
        const unsigned *w = h->q_host + (size_t)((h->q_head - h->q_count + Q_HOST_RING) % Q_HOST_RING) * sg::Q_STATE_WORDS;
        const unsigned code = w[sg::Q_ERR];
        if (code == 0 || h->q_failed) continue; // (the first give-up is the one reported)
        static const char *what[] = {"", "a rollout wavefront waited for the controller pre-pass", "a rollout wavefront waited for the previous chunk of its block",
                                     "the controller pre-pass waited for a buffer of the table ring"};
        h->q_failed = true;
        h->queue_mode = 0; // (whatever kept its wavefronts from meeting will do so again: the handle's later calls take the chunk launches)
        snprintf(h->q_msg, sizeof h->q_msg, "sg_rollout: the persistent table launch gave up (%s longer than SG_QUEUE_TIMEOUT_MS; %u work items had finished): "
                                            "the state of the batch is undefined -- sg_reset / sg_upload before the next call", what[code < 4 ? code : 0],
                 w[sg::Q_ITEMS_DONE]);
    }
    return h->q_failed ? fail(h, SG_ERR_HIP, "%s", h->q_msg) : SG_OK;
}
// sg_reset / sg_upload start the batch anew: whatever a launch before them gave up on is history
void sgh::forget_queue_failure(sg_handle *h)
{
    h->q_count = 0;
    h->q_failed = false;
}

// The table path as ONE launch (sgym_queue.hpp): the controller pre-pass and the rollout of every chunk of the time axis in one
// grid of persistent wavefronts, work items (chunk, block) from a device-side counter.  `chunk` = the longest chunk.
// Returns SG_OK, an error, or SG_QUEUE_FALLBACK: the table ring could not be allocated -- the caller takes the chunk launches.
#define SG_QUEUE_FALLBACK 1
// Wavefront slots of the persistent kernel on this device: what the build's launch bounds say (wavefronts per SIMD x SIMDs), cut
// down to what the runtime's occupancy query grants when that is less (a CU mask, a partitioned device, a build whose
// registers or LDS grew) -- every wavefront of the grid has to be resident at once, the pre-pass roles never yield.
static size_t slots_of(sg_handle *h, bool rss)
{
    const size_t by_bounds = (size_t)h->n_simd * (size_t)(rss ? SG_WAVES_PER_SIMD : (h->planar ? SG_PLANAR_WAVES : SG_TAB_WAVES));
    if (h->q_waves_G != h->G) { // (sg_upload widens the tiles of a pedestrian batch: another kernel instance, another occupancy)
        std::fill(h->q_waves_per_cu, h->q_waves_per_cu + 3, -1);
        h->q_waves_G = h->G;
    }
    int &cached = h->q_waves_per_cu[rss ? 2 : (h->planar ? 1 : 0)];
    if (cached < 0) cached = rss ? sgl::rss_tabq_waves_per_cu(h->G) : sgl::tabq_waves_per_cu(h->G, h->planar);
    return cached > 0 ? std::min(by_bounds, (size_t)cached * (size_t)(h->n_simd / 4)) : by_bounds;
}
static int launch_queue(sg_handle *h, int n_steps, int force, const double *d_actions, int chunk, size_t *ev_next, bool rss = false)
{
    const size_t nblk = h->NE / 64, np = (size_t)h->p.n_ctl_pad, n_ctl_waves = np / 64;
    // chunks of the time axis: short at first (the first rollout items cannot start before the pre-pass has written their chunk),
    // growing by ~1.4x -- the pre-pass is only 1.3 ... 1.9x faster per step than a rollout wavefront beside it, so chunk c + 1
    // has to be written in about the time chunk c takes to roll out: with lengths that doubled, a quarter of the wavefronts
    // waited through the first 4 ms (tools/dbg/queue_timeline.py) -- up to a plateau of SG_QUEUE_CAP = 512 steps (blocks are
    // at most one chunk apart, and the call ends when the LAST block does: 1024-step chunks measured 4 % slower, 256-step
    // ones 2 %, profiles/r05_ab_chunk_cap.txt), and shrinking again the same way at the end (SG_QUEUE_DECAY, percent) so that
    // the last items are short.  SG_QUEUE_GROW: the growth in percent.
    std::vector<int> len;
    chunk = std::min(chunk, std::max(1, env_int("SG_QUEUE_CAP", 512))); // (never above what the caller allows: the RSS line-test queue holds `chunk` steps)
    // (first chunk 96 / 128 / 160 / 192 / 256 steps: 94.3 / 95.9 / 97.4 / 97.2 / 95.4 G, means of four interleaved runs on one box,
    // profiles/r05_ab_first_chunk.txt -- the length also sets the last chunk's, the ramps mirror each other)
    const int first = std::max(1, std::min(chunk, env_int("SG_QUEUE_FIRST", 160)));
    const int grow = std::max(101, env_int("SG_QUEUE_GROW", 140));
    const int decay = env_int("SG_QUEUE_DECAY", 140); // 0: only the last chunk is halved (below)
    std::vector<int> up, down; // first, first * g, ... (< chunk); the mirror image at the end of the call
    for (long long n = first; n < chunk && n < chunk * 3ll / 4; n = std::max(n + 1, n * grow / 100)) up.push_back((int)n);
    if (decay > 100)
        for (long long n = first; n < chunk && n < chunk * 3ll / 4; n = std::max(n + 1, n * decay / 100)) down.insert(down.begin(), (int)n);
    long long ramp = 0;
    for (int n : up) ramp += n;
    for (int n : down) ramp += n;
    if (ramp + chunk <= n_steps) {
        // ramp up, a plateau of whole chunks, ramp down; what is left over (< chunk) goes where the ramp down reaches its length
        const long long mid = n_steps - ramp;
        const int whole = (int)(mid / chunk), rest = (int)(mid % chunk);
        len = up;
        len.insert(len.end(), (size_t)whole, chunk);
        if (rest > 0) down.insert(std::lower_bound(down.begin(), down.end(), rest, std::greater<int>()), rest);
        len.insert(len.end(), down.begin(), down.end());
    } else {
        for (int k0 = 0, n = 0; k0 < n_steps; k0 += n) {
            const long long want = len.empty() ? first : std::max<long long>((long long)len.back() + 1, (long long)len.back() * grow / 100);
            n = (int)std::min<long long>(std::min<long long>(chunk, want), n_steps - k0);
            if (want >= chunk / 2 + chunk / 4 && want < chunk) n = std::min(chunk, n_steps - k0); // (no odd chunk just below the cap)
            len.push_back(n);
        }
        while (len.size() > 1 && len.back() >= 2 * first && len.back() > 128) { // ..., L -> ..., L - L / 2, L / 2, repeated on the tail
            const int L = len.back(), half = L / 2;
            len.back() = L - half;
            len.push_back(half);
        }
    }
    const int C = (int)len.size();
    if (C > sg::Q_MAX_CHUNKS) return SG_QUEUE_FALLBACK;
    // the table ring: as many chunk buffers as the call has chunks when they fit a quarter of the free memory (no buffer is
    // ever reused: the pre-pass never waits), else a ring of at least three
    const size_t row = (size_t)sg::CT_PLANES * sg::CT_W * np;
    // (rows per lane = the longest chunk of THIS launch + 1, whatever table an earlier chunk-launch call of the handle needed:
    // the stride is a launch parameter -- ADVICE r5: a handle that once ran thousands of steps per chunk kept ring buffers of
    // that size for ever)
    const int ts = chunk;
    const size_t buf_bytes = (size_t)(ts + 1) * row * sizeof(double);
    int n_buf = C;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)8 << 30; }
        const size_t budget = std::min<size_t>((free_b + h->qtab_bytes) / 4, (size_t)std::max(1, env_int("SG_QUEUE_TAB_MB", 32768)) << 20);
        n_buf = (int)std::min<size_t>((size_t)C, std::max<size_t>(3, budget / buf_bytes));
        if (const int forced = env_int("SG_QUEUE_RING", 0)) n_buf = std::min(C, std::max(2, forced)); // (tests: a ring that is reused)
    }
    const size_t need = (size_t)n_buf * buf_bytes;
    if (need > h->qtab_bytes) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (h->d_qtab) HIP_TRY(h, hipFree(h->d_qtab));
        h->d_qtab = nullptr;
        h->qtab_bytes = 0;
        if (hipMalloc((void **)&h->d_qtab, need) != hipSuccess) {
            (void)hipGetLastError();
            h->d_qtab = nullptr;
            return SG_QUEUE_FALLBACK;
        }
        h->qtab_bytes = need;
        poison(h->stream, h->d_qtab, need);
    }
    h->p.tab_steps = ts;
    const bool q_trace = env_int("SG_QUEUE_DEBUG", 0) != 0;
    const size_t words = (size_t)sg::Q_PROG_STRIDE * (1 + n_ctl_waves) + nblk + (size_t)sg::Q_MAX_CHUNKS + 1 + (size_t)sg::Q_SEATS + (q_trace ? nblk : 0);
    if (words * sizeof(unsigned) > h->qwords.cap) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (const int rcw = h->qwords.ensure(h, words * sizeof(unsigned))) return rcw;
    }
    unsigned *const d_qwords = h->qwords.as<unsigned>();
    if (!h->q_host) HIP_TRY(h, hipHostMalloc((void **)&h->q_host, (size_t)Q_HOST_RING * sg::Q_STATE_WORDS * sizeof(unsigned), hipHostMallocDefault));
    if (h->q_count == Q_HOST_RING) { // every slot holds a launch nobody has looked at: look now
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const int rcq = check_queue(h);
        if (rcq) return rcq;
    }
    HIP_TRY(h, hipMemsetAsync(d_qwords, 0, words * sizeof(unsigned), h->stream)); // every polled word, before every launch
    sg::TabQueue tq{};
    tq.state = d_qwords;
    static_assert(sg::Q_STATE_WORDS <= sg::Q_PROG_STRIDE, "the state words have the first line to themselves");
    tq.ctl_prog = tq.state + sg::Q_PROG_STRIDE; // (one word per line, see Q_PROG_STRIDE)
    tq.blk_prog = tq.ctl_prog + (size_t)sg::Q_PROG_STRIDE * n_ctl_waves;
    tq.chunk_cnt = tq.blk_prog + nblk;
    tq.seats = tq.chunk_cnt + sg::Q_MAX_CHUNKS + 1;
    tq.trace = q_trace ? tq.seats + sg::Q_SEATS : nullptr;
    tq.defer_ticks = (long long)std::max(1, env_int("SG_QUEUE_DEFER_US", 30)) * 100ll; // 100 MHz
    tq.tab = h->d_qtab;
    tq.buf_doubles = buf_bytes / sizeof(double);
    tq.actions = d_actions;
    tq.timeout_ticks = (long long)std::max(1, env_int("SG_QUEUE_TIMEOUT_MS", 20000)) * 100000ll; // 100 MHz
    if (const int us = env_int("SG_QUEUE_TIMEOUT_US", 0)) tq.timeout_ticks = (long long)std::max(1, us) * 100ll; // (tests: a give-up on demand)
    tq.handoff = env_int("SG_QUEUE_HANDOFF", 1) != 0; // 0: a release fence per item instead (correct as well, 60 G on c3)
    tq.lag_prio = env_int("SG_QUEUE_LAGPRIO", 2);
    tq.nap = std::max(1, std::min(64, env_int("SG_QUEUE_NAP", 4))); // x 3.4 us: the longest nap between two polls of a waiting wavefront
    const char *times_path = getenv("SG_QUEUE_TIMES"); // experiment: per-item time stamps, dumped as u64 after the launch
    static unsigned long long *d_times = nullptr;
    static size_t times_cap = 0;
    const size_t n_times = (size_t)C * nblk * 4 + n_ctl_waves * (size_t)C;
    if (times_path && *times_path) {
        if (n_times > times_cap) {
            if (d_times) HIP_TRY(h, hipFree(d_times));
            HIP_TRY(h, hipMalloc((void **)&d_times, n_times * 8));
            times_cap = n_times;
        }
        HIP_TRY(h, hipMemsetAsync(d_times, 0, n_times * 8, h->stream));
        tq.times = d_times;
    }
    tq.n_chunks = C;
    tq.n_buf = n_buf;
    tq.nblk = (int)nblk;
    tq.n_ctl_waves = (int)n_ctl_waves;
    tq.k0[0] = 0;
    for (int c = 0; c < C; ++c) tq.k0[c + 1] = tq.k0[c] + len[(size_t)c];
    // as many wavefronts as the device holds at once (three per SIMD), no more than there is work for
    const size_t slots = slots_of(h, rss);
    const unsigned grid = (unsigned)std::min(slots, n_ctl_waves + nblk);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc;
    if ((rc = get_event(h, *ev_next, &e0)) || (rc = get_event(h, *ev_next + 1, &e1))) return rc;
    static hipStream_t ws = nullptr; // SG_QUEUE_DEBUG: the watcher's stream and page-locked words, made before the launch
    static unsigned *w = nullptr;
    if (q_trace && !ws) {
        HIP_TRY(h, hipStreamCreateWithFlags(&ws, hipStreamNonBlocking));
        HIP_TRY(h, hipHostMalloc((void **)&w, (sg::Q_STATE_WORDS + 16) * sizeof(unsigned), hipHostMallocDefault));
        HIP_TRY(h, hipMemcpyAsync(w, d_qwords, 64, hipMemcpyDeviceToHost, ws));
        HIP_TRY(h, hipStreamSynchronize(ws));
    }
    HIP_TRY(h, hipEventRecord(e0, h->stream));
    note_queue(h, rss);
    if (rss) sgl::rollout_rss_tabq(h->G, dim3(grid), h->stream, h->p, h->cfg.timestep, force, tq);
    else sgl::rollout_tabq(h->G, h->planar, dim3(grid), h->stream, h->p, h->cfg.timestep, force, tq);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(e1, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->q_host + (size_t)h->q_head * sg::Q_STATE_WORDS, d_qwords, sg::Q_STATE_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    h->q_head = (h->q_head + 1) % Q_HOST_RING;
    ++h->q_count;
    if (tq.times) {
        std::vector<unsigned long long> ht(n_times + 4);
        HIP_TRY(h, hipMemcpyAsync(ht.data() + 4, d_times, n_times * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        ht[0] = (unsigned long long)C; ht[1] = nblk; ht[2] = n_ctl_waves; ht[3] = grid;
        if (FILE *f = fopen(times_path, "wb")) {
            fwrite(ht.data(), 8, ht.size(), f);
            fwrite(tq.k0, sizeof(int), (size_t)C + 1, f);
            fclose(f);
        }
    }
    if (const int dbg = env_int("SG_QUEUE_DEBUG", 0)) { // watch the queue words from the host while the launch runs (dbg x 100 ms)
        fprintf(stderr, "queue: grid %u, %d chunks, ring %d, %zu blocks, %zu pre-pass wavefronts, first chunk %d steps\n", grid, C, n_buf, nblk, n_ctl_waves, len[0]);
        const int us = std::max(50, env_int("SG_QUEUE_DEBUG_US", 100000));
        const auto t_start = std::chrono::steady_clock::now();
        for (int i = 0; i < dbg; ++i) {
            std::this_thread::sleep_for(std::chrono::microseconds(us));
            if (hipMemcpyAsync(w, d_qwords, sg::Q_STATE_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, ws) != hipSuccess ||
                hipMemcpy2DAsync(w + sg::Q_STATE_WORDS, sizeof(unsigned), tq.ctl_prog, sg::Q_PROG_STRIDE * sizeof(unsigned), sizeof(unsigned),
                                 std::min<size_t>(4, n_ctl_waves), hipMemcpyDeviceToHost, ws) != hipSuccess ||
                hipStreamSynchronize(ws) != hipSuccess) break;
            fprintf(stderr, "queue +%.2f ms: tickets %u head %u err %u items done %u | ctl_prog %u %u %u %u",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(), w[0], w[1], w[2], w[3], w[8], w[9], w[10], w[11]);
            unsigned *tr = w + sg::Q_STATE_WORDS + 8;
            if (hipMemcpyAsync(tr, tq.trace, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, ws) == hipSuccess && hipStreamSynchronize(ws) == hipSuccess)
                fprintf(stderr, " | trace (chunk << 8 | stage) of blocks 0..7: %x %x %x %x %x %x %x %x", tr[0], tr[1], tr[2], tr[3], tr[4], tr[5], tr[6], tr[7]);
            fprintf(stderr, "\n");
            if (hipStreamQuery(h->stream) == hipSuccess) break;
        }
    }
    h->launch_ev.push_back((int)*ev_next);
    ++h->n_launches;
    *ev_next += 2;
    h->last_schedule = 2;
    h->last_chunks = C;
    h->last_ring = n_buf;
    h->last_grid = (int)grid;
    return SG_OK;
}

// Work of a failed call may still be running on the controller stream and the pipeline streams (the fan-out of the table
// path joins them into h->stream only at its end): wait for it, so that a later sg_synchronize / sg_upload / table regrow,
// which look at h->stream alone, never free a buffer a kernel is reading.
void sgh::drain_streams(sg_handle *h)
{
    if (h->ctl_stream) (void)hipStreamSynchronize(h->ctl_stream);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
}

// The steps of the table path: one launch on a dummy table without controlled lanes, else the persistent queue launch where it
// fits, else the chunk launches
int sgh::launch_table(sg_handle *h, const LaunchPlan &pl, int n_steps, int force, const double *d_actions, size_t *ev_next)
{
    if (pl.schedule == SCHED_TAB_DUMMY) { // nothing to integrate: the table variant reads (and ignores) one dummy row
        if (!h->d_tab[0]) {
            HIP_TRY(h, hipMalloc((void **)&h->d_tab[0], 64 * sizeof(double)));
            HIP_TRY(h, hipMalloc((void **)&h->d_tab[1], 64 * sizeof(double)));
            h->tab_bytes = 64 * sizeof(double);
            h->n_tab = 2;
            HIP_TRY(h, hipMemsetAsync(h->d_tab[0], 0, 64 * sizeof(double), h->stream));
        }
        return launch_main(h, pl, pl.fam, n_steps, 0, force, nullptr, h->d_tab[0], ev_next);
    }
    const bool no_overlap = !h->overlap;
    const size_t np = (size_t)h->p.n_ctl_pad, row = (size_t)sg::CT_PLANES * sg::CT_W * np; // doubles per step, all planes
    // chunk length: SG_CHUNK_STEPS, capped so that one table buffer stays under 1 GiB
    int ch = (int)std::min<size_t>((size_t)std::max(1, h->chunk_steps), std::max<size_t>(1, ((size_t)1 << 27) / row));
    ch = std::min(ch, n_steps);
    if (pl.rss_tab) ch = std::min(ch, std::max(1, h->rssq_steps)); // one launch fills at most the line-test queue
    // one persistent launch (sgym_queue.hpp) where the batch is one wavefront per block and nothing rides along; the
    // pre-pass role must leave most of the wavefront slots to the rollout
    int rc = SG_QUEUE_FALLBACK;
    if (h->queue_mode && h->WV == 1 && !pl.riders && !no_overlap && np / 64 <= std::min((size_t)h->n_simd, slots_of(h, pl.rss_tab)) / 2 /* a
        SIMD of its own for every pre-pass role, and at least as many rollout wavefronts resident beside them */)
        rc = launch_queue(h, n_steps, force, d_actions, ch, ev_next, pl.rss_tab);
    if (rc != SG_QUEUE_FALLBACK) return rc;
    h->last_schedule = 1;
    // The chunk launches of rounds 1-4 (crowds with riders, the RSS table variant, tiles of several wavefronts, SG_QUEUE=0):
    // the pre-pass (its own stream) writes chunk c + 1 into the second table buffer while the rollout kernel reads chunk c
    const int NB = 2; // table buffers
    const int ctl_slice = h->ctl_slice; // the pre-pass in launches of ctl_slice steps (its load then moves between SIMDs)
    if (ch > h->p.tab_steps || (size_t)(h->p.tab_steps + 1) * row * sizeof(double) > h->tab_bytes || NB > h->n_tab) {
        // grow: tab_steps + 1 rows per lane is part of the table addressing
        const int ts = std::max(ch, h->p.tab_steps);
        const size_t need = (size_t)(ts + 1) * row * sizeof(double);
        if (need > h->tab_bytes || NB > h->n_tab) { // (the buffers outlive sg_upload: the next batch of the same shape reuses them)
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->ctl_stream));
            for (int b = 0; b < 4; ++b) {
                if (h->d_tab[b]) HIP_TRY(h, hipFree(h->d_tab[b]));
                h->d_tab[b] = nullptr;
            }
            const size_t bytes = std::max(need, h->tab_bytes);
            h->tab_bytes = 0;
            h->n_tab = 0;
            for (int b = 0; b < NB; ++b) {
                HIP_TRY(h, hipMalloc((void **)&h->d_tab[b], bytes));
                poison(h->stream, h->d_tab[b], bytes);
            }
            h->tab_bytes = bytes;
            h->n_tab = NB;
        }
        h->p.tab_steps = ts;
    }
    hipStream_t cs = no_overlap ? h->stream : h->ctl_stream;
    hipEvent_t e;
    if (!no_overlap) { // the other streams start after everything queued so far (reset, uploads)
        if ((rc = get_event(h, (*ev_next)++, &e))) return rc;
        HIP_TRY(h, hipEventRecord(e, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(cs, e, 0));
    }
    const dim3 cgrid((unsigned)(np / 64));
    // chunks of the time axis: lengths double from two slices up to `ch` -- the rollout kernel cannot start before
    // the table of its chunk exists, and the pre-pass of the chunks after it (about 0.4x the rollout kernel's time
    // per step) then always finishes under the rollout kernel
    std::vector<int> ck0, cn;
    for (int k0 = 0, n = 0, c = 0; k0 < n_steps; k0 += n, ++c) {
        n = std::min(std::min(ch, c < 20 ? (2 * h->ctl_slice) << c : ch), n_steps - k0);
        ck0.push_back(k0);
        cn.push_back(n);
    }
    const int C = (int)cn.size();
    std::vector<hipEvent_t> ctl_done((size_t)C, nullptr), chunk_done((size_t)C, nullptr);
    int ctl_issued = 0;
    auto issue_ctl = [&](int upto) -> int { // the pre-pass of the chunks up to `upto`, each into buffer (chunk mod NB)
        for (; ctl_issued <= upto && ctl_issued < C; ++ctl_issued) {
            const int c = ctl_issued, k0 = ck0[(size_t)c], n = cn[(size_t)c];
            double *tab = h->d_tab[c % NB];
            if (!no_overlap && c >= NB) // the buffer is free once the rollout is through chunk c - NB
                HIP_TRY(h, hipStreamWaitEvent(cs, chunk_done[(size_t)(c - NB)], 0));
            for (int s0 = 0; s0 < n; s0 += ctl_slice)
                sgl::control(pl.ctl, cgrid, cs, h->p, h->cfg.timestep, std::min(ctl_slice, n - s0), c == 0 && s0 == 0, k0 + s0, d_actions,
                             tab, s0, pl.ctl_metrics);
            HIP_TRY(h, hipGetLastError());
            if (!no_overlap) {
                const int rc2 = get_event(h, (*ev_next)++, &ctl_done[(size_t)c]);
                if (rc2) return rc2;
                HIP_TRY(h, hipEventRecord(ctl_done[(size_t)c], cs));
            }
        }
        return SG_OK;
    };
    for (int c = 0; c < C; ++c) {
        // (chunk c + NB - 1 goes into the buffer of chunk c - 1, whose launches were queued by the previous iteration)
        if ((rc = issue_ctl(std::min(C - 1, c + NB - 1)))) return rc;
        const int b = c % NB;
        const sg::TabGroups tg = one_group(h, h->d_tab[b], cn[(size_t)c]);
        if (!no_overlap) HIP_TRY(h, hipStreamWaitEvent(h->stream, ctl_done[(size_t)c], 0));
        if ((rc = launch_main(h, pl, pl.fam, cn[(size_t)c], 0, force, nullptr, h->d_tab[b], ev_next, &tg))) return rc;
        chunk_done[(size_t)c] = h->ev_pool[*ev_next - 1];
    }
    return SG_OK;
}
