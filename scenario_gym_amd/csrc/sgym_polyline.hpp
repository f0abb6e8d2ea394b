// sgym_polyline.hpp -- Polylines as LaneSeg rows (lane centre lines, routes, driver paths; the host's append_segments builds them all)
// and the steps their kernels share: the wavefront-wide minimum of a (key, index) pair, the closest point of a segment, the best
// segment of a row range, the point at an arclength, a segment seen from a pose.  Plain unfused fp64.
// Part of the gfx950 device code of the batched rollout engine; included by sgym_device.hpp (in order: every part builds on
// the ones before it), never on its own.
#pragma once

namespace sg {

// A non-negative finite double orders as its bit pattern does, so the key of a selection is the value as a 64-bit integer,
// "no candidate" is the all-ones word, above every finite key, and an entry that holds nothing has index INDEX_NONE.
constexpr uint64_t KEY_NONE = ~0ull;
constexpr int INDEX_NONE = 0x7fffffff;

// the smallest (key, index) of the wavefront, in every lane: a butterfly of cross-lane reads, no LDS
__device__ __forceinline__ void wave_min(uint64_t &key, int &index)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint64_t ok = __shfl_xor(key, m, 64);
        const int oi = __shfl_xor(index, m, 64);
        const bool take = ok < key || (ok == key && oi < index);
        key = take ? ok : key;
        index = take ? oi : index;
    }
}

struct LaneSeg {      // one polyline segment a -> b: 80 bytes
    double ax, ay, ex, ey, L2, len, cum, bx, by; // e = b - a, L2 = ex*ex + ey*ey, len = sqrt(L2), cum = arclength of a within its polyline
    int32_t lane, first;                         // lane rows only: its lane and that lane's first segment (both indices over all networks)
};

// the closest point of segment g to (px, py): the squared distance, the offsets from that point, the effective parameter
__device__ __forceinline__ double lane_project(const LaneSeg &g, double px, double py, double &dx, double &dy, double &t)
{
    const double wx = px - g.ax, wy = py - g.ay;
    t = (wx * g.ex + wy * g.ey) / g.L2;
    double cx = g.ax, cy = g.ay;
    if (g.L2 == 0.0 || !(t > 0.0)) t = 0.0;
    else if (t >= 1.0) { t = 1.0; cx = g.bx; cy = g.by; }
    else { cx = g.ax + t * g.ex; cy = g.ay + t * g.ey; }
    dx = px - cx; dy = py - cy;
    return dx * dx + dy * dy;
}

// The segment of the rows [s0, s1) closest to (px, py), for a whole wavefront: its index within the range, the same in every
// lane, or -1 (no rows, or no finite distance: a NaN fails).  The lanes stride over the rows (a load is 64 consecutive 80-byte
// rows, the index clamped to the last row) and keep the smallest (d2 bits, index) with a strict <, so ascending indices per
// lane let the lower index keep a tie; wave_min makes it the wavefront's.
__device__ __forceinline__ int polyline_nearest(const LaneSeg *seg, int s0, int s1, int lane, double px, double py)
{
    uint64_t bk = KEY_NONE;
    int bi = INDEX_NONE;
    for (int i0 = s0; i0 < s1; i0 += 64) {
        const int i = i0 + lane;
        const LaneSeg g = seg[min(i, s1 - 1)];
        double dx, dy, t;
        const double d2 = lane_project(g, px, py, dx, dy, t);
        const bool take = i < s1 && d2 < __builtin_inf() && (uint64_t)__double_as_longlong(d2) < bk;
        bk = take ? (uint64_t)__double_as_longlong(d2) : bk;
        bi = take ? i - s0 : bi;
    }
    wave_min(bk, bi);
    return bk == KEY_NONE ? -1 : bi;
}

// the point at arclength `target` of the polyline rows [s0, s1) (s0 < s1) whose length is `total`; beyond the end: its last point
__device__ __forceinline__ void polyline_point_at(const LaneSeg *seg, int s0, int s1, double total, double target, double &x, double &y)
{
    if (target > total) { x = seg[s1 - 1].bx; y = seg[s1 - 1].by; return; }
    int lo = s0, hi = s1; // the last segment with cum <= target (cum[s0] = 0 <= target)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid].cum <= target) lo = mid; else hi = mid;
    }
    const LaneSeg g = seg[lo];
    const double u = g.len == 0.0 ? 0.0 : (target - g.cum) / g.len;
    if (u >= 1.0) { x = g.bx; y = g.by; }
    else { x = g.ax + u * g.ex; y = g.ay + u * g.ey; }
}

// segment g seen from the pose (px, py) with heading (s, c): the squared distance to its closest point, the lateral offset (left
// of the segment's direction positive), cos and sin of the heading against that direction (all three zero for a segment of
// length zero, which has none), the arclength of the closest point, the offset along the segment's direction (rounding noise
// unless the closest point is an end of the segment), and that direction
struct SegmentView { double d2, offset, cos_err, sin_err, arc, along, ux, uy; };
__device__ __forceinline__ SegmentView segment_view(const LaneSeg &g, double px, double py, double s, double c)
{
    double dx, dy, t;
    SegmentView v;
    v.d2 = lane_project(g, px, py, dx, dy, t);
    const double ux = g.len == 0.0 ? 0.0 : g.ex / g.len, uy = g.len == 0.0 ? 0.0 : g.ey / g.len;
    v.offset = ux * dy - uy * dx;
    v.cos_err = c * ux + s * uy;
    v.sin_err = s * ux - c * uy;
    v.arc = g.cum + t * g.len;
    v.along = ux * dx + uy * dy;
    v.ux = ux;
    v.uy = uy;
    return v;
}

} // namespace sg
