// sgym_policy.hpp -- driver_policy_kernel: the built-in driver policy, an IDM car-follower along a path, for the listed drivers of
// sg_set_driver_policy (no counterpart in the reference, whose agents are replay, PID, pedestrian or caller-run).
//
// The kernel turns the current state into one (accel, steer) per policy driver; drive_kernel (sgym_drive.hpp) consumes the pair like a
// caller's.  The definition is in include/sgym.h at sg_set_driver_policy: plain unfused fp64 with IEEE division and square root.
// The path rows are LaneSeg rows built by sg_set_driver_policy exactly as sg_set_lanes builds its own, read through polyline_nearest
// and segment_view (sgym_polyline.hpp); the driver is an Observer and the scenario's slots are observed_slot's (sgym_observers.hpp).
// PolicyIndex is what the host units keep (sgym_launch.hpp includes this header); the kernel is emitted by k_drive.hip alone.
#pragma once
#include "sgym_device.hpp"

namespace sg {

struct PolicyIndex {      // device pointers, by value; driver == nullptr: no policy set
    const int32_t *driver;  // [m] positions in the driver list, strictly ascending
    const int32_t *seg_off; // [m + 1] ranges of seg
    const double *params;   // [m][SG_DP_NPARAM]
    const double *total;    // [m] cum + len of the path's last segment (0 without segments)
    const LaneSeg *seg;     // the segments of every path, path by path
    int64_t n_along;        // how many of the m rows have SG_DP_CORRIDOR == 1: which instantiations of the kernel a launch needs
};

// the box of the entity with the rows (d, st) as the policy reads it: its centre, sin and cos of its heading, its width and length
struct PolicyBox {
    double qx, qy, sn, cn, W, L;
};

__device__ __forceinline__ PolicyBox policy_box(const double *d, const double *st)
{
    PolicyBox b;
    sg_sincos(d[(SG_F_POSE + 3) * 64], b.sn, b.cn);
    b.W = st[ST_BW * 64];
    b.L = st[ST_BL * 64];
    const double cxe = st[ST_BCX * 64], cye = st[ST_BCY * 64];
    b.qx = d[(SG_F_POSE + 0) * 64] + (cxe * b.cn - cye * b.sn);
    b.qy = d[(SG_F_POSE + 1) * 64] + (cxe * b.sn + cye * b.cn);
    return b;
}

// what the policy asks of a box as a lead: the longitudinal and lateral offset of its centre and its half extents along and across,
// all in one frame -- the heading frame of driver f (the straight corridor), or the frame of a path segment (the corridor along the
// path: arclength and lateral offset relative to the driver's own; `along` and the segment's direction come with it)
struct PolicyLead {
    double lon, lat, hl, hw;
};

__device__ __forceinline__ void policy_extents(const PolicyBox &b, double cr, double sr, PolicyLead &q)
{
    q.hl = 0.5 * (__builtin_fabs(b.L * cr) + __builtin_fabs(b.W * sr));
    q.hw = 0.5 * (__builtin_fabs(b.L * sr) + __builtin_fabs(b.W * cr));
}

__device__ __forceinline__ PolicyLead policy_lead(const double *d, const double *st, const Observer &f)
{
    const PolicyBox b = policy_box(d, st);
    double cr, sr;
    f.to_frame(b.cn, b.sn, cr, sr);
    PolicyLead q;
    f.to_frame(b.qx - f.x, b.qy - f.y, q.lon, q.lat);
    policy_extents(b, cr, sr, q);
    return q;
}

// the box seen from path segment g, for a driver at arclength s0 and lateral offset off of its own best segment
__device__ __forceinline__ PolicyLead policy_lead_on(const LaneSeg &g, const PolicyBox &b, double s0, double off, SegmentView &sv)
{
    sv = segment_view(g, b.qx, b.qy, b.sn, b.cn);
    PolicyLead q;
    policy_extents(b, sv.cos_err, sv.sin_err, q);
    q.lon = sv.arc - s0;
    q.lat = sv.offset - off;
    return q;
}

// a value that is the same in every lane, told to the compiler: it then lives in scalar registers and a branch on it is uniform
__device__ __forceinline__ double wave_uniform(double v)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// The window of the corridor along the path: the rows [g0, g1) of the driver's path from its own best segment on, as far as
// cum <= bound (cum never decreases, so the first row beyond the bound ends the loop: the bound is the trip count, which is what
// keeps a recording of a thousand points affordable).  g0, g1 and bound are wavefront-uniform: the rows come by scalar loads, one
// row for all 64 lanes, and each lane projects its own point.  Returns the row with the smallest (d2, index), -1 when there is
// none (an empty window, or no finite distance).
__device__ __forceinline__ int policy_window_nearest(const LaneSeg *seg, int g0, int g1, double bound, double px, double py)
{
    double bd = __builtin_inf();
    int bi = -1;
    if (g0 >= g1) return bi;
    LaneSeg g = seg[g0];
    for (int i = g0; i < g1; ++i) {
        const LaneSeg next = seg[i + 1 < g1 ? i + 1 : i]; // (asked for a row ahead: a path of a thousand rows comes from memory, not from a cache)
        if (!(g.cum <= bound)) break;
        double dx, dy, t;
        const double d2 = lane_project(g, px, py, dx, dy, t);
        const bool take = d2 < bd; // (finite, then: a NaN fails; ascending rows: the lower index keeps a tie)
        bd = take ? d2 : bd;
        bi = take ? i : bi;
        g = next;
    }
    return bi;
}

// a double as a 64-bit key that orders as the value does, negative values included (-0.0 is brought to +0.0 first: equal values
// must tie); NaNs never get here
__device__ __forceinline__ uint64_t policy_signed_key(double g)
{
    const uint64_t b = (uint64_t)__double_as_longlong(g == 0.0 ? 0.0 : g);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

// Policy driver o < m: driver P.driver[o] of the list (scen, slot).  actions: the pair of o goes to row (row_of ? row_of[o] : o) of
// [..][2]; info [m][SG_DP_NINFO] (may be nullptr), feat [m][SG_DP_NFEAT] (may be nullptr); every byte of the rows is written.
// One wavefront per policy driver, four per workgroup, no LDS, no barrier, no atomics.  What belongs to the driver alone is the same
// in every lane: each lane loads and computes it for itself (Observer, sgym_observers.hpp).
//   phase one, lane = path segment: polyline_nearest.  Every lane then projects onto the best row again (segment_view): the same
//     operations on the same operands, so the same bits.
//   phase two, lane = entity: the scenario's slots go by in blocks of 64, ascending (any scenario width); per lane a running
//     (gap key, slot) with a strict <, then wave_min.  The gap is signed, so its key is policy_signed_key.  Every lane then
//     computes the lead's terms again for gap and dv.
//     An instantiation per mode: a policy of one mode (PolicyIndex::n_along is 0 or m) launches that one, which asks nothing;
//     a MIXED one launches both, each taking the rows of its mode and leaving the others at once.  <false> is the straight rule alone, with the registers it had before the other rule existed
//     (71 VGPRs against 85: seven wavefronts per SIMD against five); <true> measures the lead along the path instead: every
//     lane walks the window of the driver's path for its entity (policy_window_nearest: scalar row loads, no LDS), loads its best
//     row, and views its box from there (segment_view); the lane also keeps the row of its running lead, which the winner's lane
//     hands to the wavefront.  A block of 64 slots with nobody in the scene skips the walk.
//   then the law, and lanes 0..5 store.
#ifdef SG_UNIT_DRIVE // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
template <bool ALONG, bool MIXED>
static __global__ __launch_bounds__(256) void driver_policy_kernel(Params p, PolicyIndex P, const int32_t *scen, const int32_t *slot, int64_t m,
                                                                   const int32_t *row_of, double *actions, int32_t *info, double *feat)
{
    int lane; int64_t o;
    if (!wave_item(m, lane, o)) return; // (the whole wavefront, which meets no barrier)
    const double *prm = P.params + (size_t)o * SG_DP_NPARAM;
    if constexpr (MIXED)
        if ((prm[SG_DP_CORRIDOR] != 0.0) != ALONG) return; // (the other instantiation's row)
    const int drv = P.driver[o];
    const Observer f = observer_at(p, scen[drv], slot[drv]);
    double *act = actions + (size_t)(row_of ? row_of[o] : (int32_t)o) * 2;
    if (!f.present) { // not in State.poses: drive_kernel does with it what it does today
        if (lane < 2) act[lane] = 0.0;
        if (info && lane < SG_DP_NINFO) info[(size_t)o * SG_DP_NINFO + lane] = -1;
        if (feat && lane < SG_DP_NFEAT) feat[(size_t)o * SG_DP_NFEAT + lane] = 0.0;
        return;
    }
    const ObservedSlot own = observed_slot(p, f, f.slot);
    const double *st = own.stat, v = own.dyn[(SG_F_CTRL + 0) * 64];
    const double Wo = st[ST_BW * 64], cyo = st[ST_BCY * 64], front = st[ST_BCX * 64] + 0.5 * st[ST_BL * 64];

    // the path term
    const int s0i = P.seg_off[o], best = polyline_nearest(P.seg, s0i, P.seg_off[o + 1], lane, f.x, f.y);
    const bool on_path = best >= 0;
    double steer = 0.0, off = 0.0, se = 0.0, arc = 0.0, rem = __builtin_inf();
    if (on_path) {
        const SegmentView sv = segment_view(P.seg[s0i + best], f.x, f.y, f.s, f.c);
        off = sv.offset;
        se = sv.sin_err;
        if (sv.cos_err < 0.0) se = se >= 0.0 ? 1.0 : -1.0;
        arc = sv.arc;
        rem = P.total[o] - arc;
        steer = -(prm[SG_DP_K_PSI] * se + (prm[SG_DP_K_E] * off) / (prm[SG_DP_K_SOFT] + __builtin_fabs(v)));
    }

    // the lead
    const double half = prm[SG_DP_HALF], reach = prm[SG_DP_REACH];
    const double left = (cyo + 0.5 * Wo) + half, right = (cyo - 0.5 * Wo) - half;
    uint64_t lk = KEY_NONE;
    int ls = INDEX_NONE;
    double gap = __builtin_inf(), dv = 0.0;
    bool lead;
    const int g0 = s0i + __builtin_amdgcn_readfirstlane(best);
    bool along = false;
    if constexpr (ALONG) along = g0 >= s0i; // (without a best segment: the straight rule)
    if (along) { // the corridor along the path (the same branch in every lane)
        const int g1 = P.seg_off[o + 1];
        const double bound = wave_uniform((arc + front) + reach);
        int lg = g0; // the best window row of this lane's running lead
        for (int e0 = 0; e0 < p.E; e0 += 64) {
            const int e = e0 + lane;
            const ObservedSlot es = observed_slot(p, f, e);
            const bool there = es.other && es.present();
            if (!sg_any(there)) continue; // (a block with nobody in the scene: no pass over the window)
            const PolicyBox b = policy_box(es.dyn, es.stat);
            const int k = policy_window_nearest(P.seg, g0, g1, bound, b.qx, b.qy);
            const LaneSeg g = P.seg[k < 0 ? g0 : k];
            SegmentView sv;
            const PolicyLead q = policy_lead_on(g, b, arc, off, sv);
            const double ge = (q.lon - q.hl) - front;
            const bool in = there && k >= 0 && g.len != 0.0 && q.lat - q.hw <= left && q.lat + q.hw >= right && q.lon + q.hl > front &&
                            ge <= reach && __builtin_fabs(sv.along) <= q.hl; // (a NaN anywhere fails)
            const uint64_t key = in ? policy_signed_key(ge) : KEY_NONE;
            const bool take = key < lk; // (ascending slots per lane: the lower slot keeps a tie)
            lk = take ? key : lk;
            ls = take ? e : ls;
            lg = take ? k : lg;
        }
        wave_min(lk, ls);
        lead = lk != KEY_NONE;
        const int k = __shfl(lg, ls & 63, 64); // (slot ls was lane ls & 63's)
        if (lead) {
            const ObservedSlot es = observed_slot(p, f, ls);
            SegmentView sv;
            const PolicyLead q = policy_lead_on(P.seg[k], policy_box(es.dyn, es.stat), arc, off, sv);
            gap = (q.lon - q.hl) - front;
            dv = v - (es.dyn[(SG_F_VEL + 0) * 64] * sv.ux + es.dyn[(SG_F_VEL + 1) * 64] * sv.uy);
        }
    } else { // the straight corridor, in the driver's heading frame
        for (int e0 = 0; e0 < p.E; e0 += 64) {
            const int e = e0 + lane;
            const ObservedSlot es = observed_slot(p, f, e);
            const PolicyLead q = policy_lead(es.dyn, es.stat, f);
            const double ge = (q.lon - q.hl) - front;
            const bool in = es.other && es.present() && q.lat - q.hw <= left && q.lat + q.hw >= right && q.lon + q.hl > front &&
                            ge <= reach; // (a NaN anywhere fails)
            const uint64_t key = in ? policy_signed_key(ge) : KEY_NONE;
            const bool take = key < lk; // (ascending slots per lane: the lower slot keeps a tie)
            lk = take ? key : lk;
            ls = take ? e : ls;
        }
        wave_min(lk, ls);
        lead = lk != KEY_NONE;
        if (lead) {
            const ObservedSlot es = observed_slot(p, f, ls);
            const PolicyLead q = policy_lead(es.dyn, es.stat, f);
            gap = (q.lon - q.hl) - front;
            dv = v - (es.dyn[(SG_F_VEL + 0) * 64] * f.c + es.dyn[(SG_F_VEL + 1) * 64] * f.s);
        }
    }

    // the acceleration
    const double A = prm[SG_DP_A], T = prm[SG_DP_T], S0 = prm[SG_DP_S0], gap_min = prm[SG_DP_GAP_MIN];
    const double vr = v / prm[SG_DP_V0], free_ = 1.0 - (vr * vr) * (vr * vr);
    const double root = 2.0 * __builtin_sqrt(A * prm[SG_DP_B]);
    const auto idm = [&](double g, double dd) {
        const double q = v * T + (v * dd) / root;
        const double ss = S0 + (q > 0.0 ? q : 0.0);
        const double gg = g > gap_min ? g : gap_min;
        const double rr = ss / gg;
        return A * (free_ - rr * rr);
    };
    double acc = lead ? idm(gap, dv) : A * free_;
    if (on_path) {
        const double ae = idm(rem, v);
        acc = ae < acc ? ae : acc;
    }

    if (lane < 2) act[lane] = lane == 0 ? acc : steer;
    if (info && lane < SG_DP_NINFO) info[(size_t)o * SG_DP_NINFO + lane] = lane == 0 ? (lead ? ls : -1) : best;
    if (feat && lane < SG_DP_NFEAT)
        feat[(size_t)o * SG_DP_NFEAT + lane] = lane == 0 ? gap : lane == 1 ? dv : lane == 2 ? off : lane == 3 ? se : lane == 4 ? arc : rem;
}
#endif // SG_UNIT_DRIVE

} // namespace sg
