// sgym_geom.hpp -- Which road geometries contain a point: RoadNetwork.get_geometries_at_point / State.get_road_info_at_entity.
// Part of the gfx950 device code of the batched rollout engine; included by sgym_device.hpp (in order: every part builds on
// the ones before it), never on its own.
#pragma once

namespace sg {

// ------------------------------------------------------------------------------------------------
// road_network.py:375-407: `[x for x in road_network_geometries if x.boundary.contains(Point(px, py))]` -- every polygon on
// its own (strictly inside its exterior ring and outside its holes; on a ring: not contained), whatever its SG_LAYER_* bits.
// The reference tests every geometry for every point.  Here the cell grid of sgym_road.hpp answers, with a second list per
// cell beside the layer words: the polygons that have anything to say about the cell, ascending, each entry either
//   RG_FULL   the polygon covers the WHOLE cell (its boundary does not come near it): contained, nothing to test
//   RG_CAND   entry of RoadIndex::cand: the polygon's boundary touches the cell -- rn_locate_in_cell on its edges there
//   RG_XCAND  the same for a polygon without layer bits, which the layer index skips (its own candidate array: the arrays
//             the layer kernels read stay as they are)
// so a point costs the entries of its one cell.  The predicates are those of sgym_road.hpp: the answer is the exact one for
// the fp64 coordinates given.
// ------------------------------------------------------------------------------------------------
enum { RG_FULL = 0, RG_CAND = 1, RG_XCAND = 2, RG_SHIFT = 30 };
struct RoadGeom {
    const uint32_t *ref_off;      // CSR over all cells of all networks (the cell numbering of RoadIndex::cell_off)
    const uint32_t *ref;          // kind << RG_SHIFT | index: polygon (RG_FULL), entry of cand (RG_CAND) / xcand (RG_XCAND)
    const RoadCand *xcand;        // boundary candidates of the polygons without layer bits
    const int32_t *xcand_edges;   // their edge lists (indices into RoadIndex::edges)
    const int32_t *poly0;         // [n_nets] first polygon of each network: results are network-local indices
};

// The geometries of network `net` that contain (px, py): returns how many (it may exceed cap), writes the first `cap` of
// their network-local indices to geoms (ascending; nullptr: none are written) and the OR of ALL their layer bits to `layers`.
__host__ __device__ inline int rn_geoms_at(const RoadIndex &R, const RoadGeom &G, int net, double px, double py, int cap,
                                           int32_t *geoms, uint32_t &layers)
{
    layers = 0u;
    if (net < 0) return 0;
    const RoadNet N = R.nets[net];
    int ix, iy;
    if (!rn_cell_of(N, px, py, ix, iy)) return 0;
    const int64_t cell = N.cell_base + (int64_t)iy * N.nx + ix;
    const uint32_t k0 = G.ref_off[cell], k1 = G.ref_off[cell + 1];
    const int32_t q0 = G.poly0[net];
    int n = 0;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t code = G.ref[k], kind = code >> RG_SHIFT, idx = code & ((1u << RG_SHIFT) - 1u);
        int32_t poly = (int32_t)idx;
        if (kind != RG_FULL) {
            const RoadCand cd = kind == RG_CAND ? R.cand[idx] : G.xcand[idx];
            const int32_t *list = (kind == RG_CAND ? R.cand_edges : G.xcand_edges) + cd.edge_off;
            double rx, ry;
            rn_ref_point(N, ix, iy, cd.ref_sel, rx, ry);
            if (rn_locate_in_cell(R.edges, list, cd.n_edges, rx, ry, cd.ref_inside != 0, px, py) != 1) continue;
            poly = cd.poly;
        }
        layers |= R.poly_layers[poly];
        if (geoms && n < cap) geoms[n] = poly - q0;
        ++n;
    }
    return n;
}

// One lane per query.  xy == nullptr: query t = entity slot (r, e) = (t / E, t % E) at its current pose, read from the state
// blocks (entity r * EP + e of `dyn`, the one layout of every width); count = -1 for a slot that is not in State.poses (the
// reference raises KeyError).  Else: the point xy[t] of scenario scen[t].  has_road == 0 (no networks set) and scenarios
// without a network: count = 0, as state.py:334-335 returns ([], []).  geoms / layers may be nullptr.
#ifdef SG_UNIT_GEOM // (emitted by the one object that launches it: csrc/Makefile, sgym_launch.hpp)
static __global__ __launch_bounds__(256) void road_info_kernel(const double *dyn, int E, int EP, int FROWS, RoadIndex R, RoadGeom G,
                                                               int has_road, const int32_t *scen, const double *xy, int64_t n, int cap,
                                                               int32_t *count, int32_t *geoms, uint32_t *layers)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    int r;
    double px, py;
    bool present = true;
    if (xy) {
        r = scen[t];
        px = xy[2 * t];
        py = xy[2 * t + 1];
    } else {
        r = (int)(t / E);
        const uint32_t idx = (uint32_t)r * (uint32_t)EP + (uint32_t)(t - (int64_t)r * E);
        const double *row = dyn + (size_t)(idx >> 6) * ((size_t)FROWS * 64) + (idx & 63);
        present = *reinterpret_cast<const uint64_t *>(row + SG_F_PRESENT * 64) != 0;
        px = row[(SG_F_POSE + 0) * 64];
        py = row[(SG_F_POSE + 1) * 64];
    }
    int32_t *mine = geoms ? geoms + t * (int64_t)cap : nullptr;
    uint32_t L = 0u;
    int c = -1;
    if (present) c = rn_geoms_at(R, G, has_road ? R.net_of_scen[r] : -1, px, py, cap, mine, L);
    if (mine)
        for (int k = c < 0 ? 0 : c; k < cap; ++k) mine[k] = -1;
    count[t] = c;
    if (layers) layers[t] = L;
}
#endif // SG_UNIT_GEOM

} // namespace sg
