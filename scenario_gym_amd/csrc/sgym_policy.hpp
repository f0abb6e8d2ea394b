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
};

// what the policy asks of the entity with the rows (d, st) as a lead of driver f: the longitudinal and lateral offset of its box
// centre in the driver's frame, and the half extents of its box along and across the driver's heading
struct PolicyLead {
    double lon, lat, hl, hw;
};

__device__ __forceinline__ PolicyLead policy_lead(const double *d, const double *st, const Observer &f)
{
    double sn, cn;
    sg_sincos(d[(SG_F_POSE + 3) * 64], sn, cn);
    const double We = st[ST_BW * 64], Le = st[ST_BL * 64], cxe = st[ST_BCX * 64], cye = st[ST_BCY * 64];
    const double qx = d[(SG_F_POSE + 0) * 64] + (cxe * cn - cye * sn), qy = d[(SG_F_POSE + 1) * 64] + (cxe * sn + cye * cn);
    double cr, sr;
    f.to_frame(cn, sn, cr, sr);
    PolicyLead q;
    f.to_frame(qx - f.x, qy - f.y, q.lon, q.lat);
    q.hl = 0.5 * (__builtin_fabs(Le * cr) + __builtin_fabs(We * sr));
    q.hw = 0.5 * (__builtin_fabs(Le * sr) + __builtin_fabs(We * cr));
    return q;
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
//   then the law, and lanes 0..5 store.
#ifdef SG_UNIT_DRIVE // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void driver_policy_kernel(Params p, PolicyIndex P, const int32_t *scen, const int32_t *slot, int64_t m,
                                                                   const int32_t *row_of, double *actions, int32_t *info, double *feat)
{
    int lane; int64_t o;
    if (!wave_item(m, lane, o)) return; // (the whole wavefront, which meets no barrier)
    const int drv = P.driver[o];
    const Observer f = observer_at(p, scen[drv], slot[drv]);
    double *act = actions + (size_t)(row_of ? row_of[o] : (int32_t)o) * 2;
    if (!f.present) { // not in State.poses: drive_kernel does with it what it does today
        if (lane < 2) act[lane] = 0.0;
        if (info && lane < SG_DP_NINFO) info[(size_t)o * SG_DP_NINFO + lane] = -1;
        if (feat && lane < SG_DP_NFEAT) feat[(size_t)o * SG_DP_NFEAT + lane] = 0.0;
        return;
    }
    const double *prm = P.params + (size_t)o * SG_DP_NPARAM;
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
    for (int e0 = 0; e0 < p.E; e0 += 64) {
        const int e = e0 + lane;
        const ObservedSlot es = observed_slot(p, f, e);
        const PolicyLead q = policy_lead(es.dyn, es.stat, f);
        const double gap = (q.lon - q.hl) - front;
        const bool in = es.other && es.present() && q.lat - q.hw <= left && q.lat + q.hw >= right && q.lon + q.hl > front &&
                        gap <= reach; // (a NaN anywhere fails)
        const uint64_t key = in ? policy_signed_key(gap) : KEY_NONE;
        const bool take = key < lk; // (ascending slots per lane: the lower slot keeps a tie)
        lk = take ? key : lk;
        ls = take ? e : ls;
    }
    wave_min(lk, ls);
    const bool lead = lk != KEY_NONE;
    double gap = __builtin_inf(), dv = 0.0;
    if (lead) {
        const ObservedSlot es = observed_slot(p, f, ls);
        const PolicyLead q = policy_lead(es.dyn, es.stat, f);
        gap = (q.lon - q.hl) - front;
        dv = v - (es.dyn[(SG_F_VEL + 0) * 64] * f.c + es.dyn[(SG_F_VEL + 1) * 64] * f.s);
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
