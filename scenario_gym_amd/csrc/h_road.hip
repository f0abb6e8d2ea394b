// h_road.hip -- road networks: the cell index built on the host, the lane centre lines, and which road geometries contain each
// entity / point (delivered through deliver() and scratch(), sgym_host.hpp).
#include "sgym_host.hpp"

using namespace sgh;

// ---- road surfaces -------------------------------------------------------------------------------
// Index of one network: a uniform grid; per polygon the cells its edges touch (boxes grown by a margin far above the
// rounding of the device's cell lookup) become candidates of that polygon, the other cells of its bounding box are
// wholly inside or wholly outside -- decided with the exact test at the cell centre, once per run of untouched cells.
namespace {
struct RoadBuild {
    std::vector<sg::RoadNet> nets;
    std::vector<uint16_t> cells;
    std::vector<uint32_t> cell_off;
    std::vector<sg::RoadCand> cand;
    std::vector<int32_t> cand_edges;
    std::vector<double> edges;
    std::vector<int64_t> poly_edge_off;
    std::vector<uint32_t> poly_layers;
    std::vector<uint32_t> net_flags;   // bit 0: walkable surface has area, bit 1: impenetrable surface has area
    std::vector<int64_t> imp_off;      // per network: range of imp_edges
    std::vector<double> imp_edges;     // the ring edges of the impenetrable polygons, polygon by polygon
    // sg::RoadGeom (sgym_geom.hpp): per cell the polygons that cover it or touch it, by name
    std::vector<uint32_t> ref_off, ref;
    std::vector<sg::RoadCand> xcand;   // candidates of the polygons without layer bits (the layer index above skips them)
    std::vector<int32_t> xcand_edges;
    std::vector<int32_t> poly0;
};

int build_road_network(const sg_road_networks *in, int n, RoadBuild &B)
{
    const int64_t q0 = in->poly_off[n], q1 = in->poly_off[n + 1];
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    uint32_t flags = 0;
    for (int64_t q = q0; q < q1; ++q) {
        for (int64_t r = in->ring_off[q]; r < in->ring_off[q + 1]; ++r) {
            const int64_t a = in->vert_off[r], b = in->vert_off[r + 1];
            for (int64_t i = a; i < b; ++i) {
                const int64_t j = i + 1 < b ? i + 1 : a;
                const double *v = in->verts + 2 * i, *w = in->verts + 2 * j;
                B.edges.insert(B.edges.end(), {v[0], v[1], w[0], w[1]});
                for (int c = 0; c < 2; ++c) { lo[c] = std::min(lo[c], v[c]); hi[c] = std::max(hi[c], v[c]); }
            }
        }
        B.poly_edge_off.push_back((int64_t)B.edges.size() / 4);
        B.poly_layers.push_back(in->layers[q]);
        {   // `surface.area > 0` (social_force.py:87, 97) and the edge list the nearest-point search walks
            const int64_t e0 = B.poly_edge_off[B.poly_edge_off.size() - 2], e1 = B.poly_edge_off.back();
            double a2 = 0.0;
            for (int64_t i = e0; i < e1; ++i) a2 += B.edges[4 * i] * B.edges[4 * i + 3] - B.edges[4 * i + 2] * B.edges[4 * i + 1];
            if (a2 != 0.0 && (in->layers[q] & SG_LAYER_WALKABLE)) flags |= 1u;
            if (a2 != 0.0 && (in->layers[q] & SG_LAYER_IMPENETRABLE)) flags |= 2u;
            if (in->layers[q] & SG_LAYER_IMPENETRABLE) B.imp_edges.insert(B.imp_edges.end(), B.edges.begin() + 4 * e0, B.edges.begin() + 4 * e1);
        }
    }
    B.net_flags.push_back(flags);
    B.imp_off.push_back((int64_t)B.imp_edges.size() / 4);
    sg::RoadNet N{};
    N.cell_base = (int64_t)B.cells.size();
    const int64_t gq0 = (int64_t)B.poly_layers.size() - (q1 - q0);
    B.poly0.push_back((int32_t)gq0);
    if (!(lo[0] <= hi[0])) { // no geometry: an empty 1 x 1 grid
        N.x0 = N.y0 = 0.0; N.inv_cell = 1.0; N.nx = N.ny = 1;
        B.nets.push_back(N);
        B.cells.push_back(0);
        B.cell_off.push_back((uint32_t)B.cand.size());
        B.ref_off.push_back((uint32_t)B.ref.size());
        return 0;
    }
    double c = 1.0; // cell side: 1 m unless the network is so large that this would take more than 2^21 cells
    while (((hi[0] - lo[0]) / c + 4) * ((hi[1] - lo[1]) / c + 4) > 2097152.0) c *= 2;
    const double eps = 1e-6; // >> rounding of (p - x0) * inv_cell for coordinates below 1e9 cells
    N.x0 = std::floor(lo[0] / c) * c - c;
    N.y0 = std::floor(lo[1] / c) * c - c;
    N.inv_cell = 1.0 / c;
    N.nx = (int32_t)std::ceil((hi[0] - N.x0) / c) + 2;
    N.ny = (int32_t)std::ceil((hi[1] - N.y0) / c) + 2;
    const size_t ncell = (size_t)N.nx * N.ny;
    B.cells.resize((size_t)N.cell_base + ncell, 0);
    uint16_t *cells = B.cells.data() + N.cell_base;
    struct Entry { uint32_t cell; sg::RoadCand cd; };
    std::vector<Entry> entries, xentries; // candidates of this network (x: of its polygons without layer bits), sorted by cell below
    struct GRef { uint32_t cell; int32_t poly; uint32_t code; };
    std::vector<GRef> grefs;    // the per-geometry lists of this network's cells (sg::RoadGeom), sorted by (cell, polygon) below
    auto cix = [&](double x, double x0, int nmax) { return std::max(0, std::min(nmax - 1, (int)std::floor((x - x0) / c))); };
    std::vector<uint8_t> touched;
    std::vector<std::pair<uint32_t, int32_t>> hits; // (local cell, edge) of one polygon
    for (int64_t q = q0; q < q1; ++q) {
        const int64_t gq = gq0 + (q - q0);
        const int64_t e0 = B.poly_edge_off[gq], e1 = B.poly_edge_off[gq + 1];
        const uint32_t L = B.poly_layers[gq] & 0xffu;
        if (e1 <= e0) continue;
        // (a polygon without layer bits changes nothing the layer kernels read: its candidates go to xcand, and L = 0 leaves
        // the cell words as they are)
        std::vector<int32_t> &edge_lists = L ? B.cand_edges : B.xcand_edges;
        double plo[2] = {INFINITY, INFINITY}, phi[2] = {-INFINITY, -INFINITY};
        for (int64_t i = e0; i < e1; ++i)
            for (int c2 = 0; c2 < 2; ++c2) { plo[c2] = std::min(plo[c2], B.edges[4 * i + c2]); phi[c2] = std::max(phi[c2], B.edges[4 * i + c2]); }
        const int ix0 = cix(plo[0] - eps, N.x0, N.nx), ix1 = cix(phi[0] + eps, N.x0, N.nx);
        const int iy0 = cix(plo[1] - eps, N.y0, N.ny), iy1 = cix(phi[1] + eps, N.y0, N.ny);
        const int w = ix1 - ix0 + 1, hgt = iy1 - iy0 + 1;
        touched.assign((size_t)w * hgt, 0);
        hits.clear();
        for (int64_t i = e0; i < e1; ++i) {
            const double ax = B.edges[4 * i], ay = B.edges[4 * i + 1], bx = B.edges[4 * i + 2], by = B.edges[4 * i + 3];
            const int jx0 = cix(std::min(ax, bx) - eps, N.x0, N.nx), jx1 = cix(std::max(ax, bx) + eps, N.x0, N.nx);
            const int jy0 = cix(std::min(ay, by) - eps, N.y0, N.ny), jy1 = cix(std::max(ay, by) + eps, N.y0, N.ny);
            for (int iy = jy0; iy <= jy1; ++iy)
                for (int ix = jx0; ix <= jx1; ++ix) {
                    // the grown cell box and the segment overlap in x and in y (by the ranges above); they are disjoint
                    // iff the box lies strictly on one side of the segment's line
                    const double bx0 = N.x0 + ix * c - eps, bx1 = N.x0 + (ix + 1) * c + eps;
                    const double by0 = N.y0 + iy * c - eps, by1 = N.y0 + (iy + 1) * c + eps;
                    const double dx = bx - ax, dy = by - ay;
                    const double d0 = dx * (by0 - ay) - dy * (bx0 - ax), d1 = dx * (by0 - ay) - dy * (bx1 - ax);
                    const double d2 = dx * (by1 - ay) - dy * (bx0 - ax), d3 = dx * (by1 - ay) - dy * (bx1 - ax);
                    const double tol = 1e-9 * (std::fabs(dx) + std::fabs(dy)) * (c + std::fabs(bx0 - ax) + std::fabs(by0 - ay) + 1.0);
                    const double mn = std::min(std::min(d0, d1), std::min(d2, d3)), mx = std::max(std::max(d0, d1), std::max(d2, d3));
                    if (mn > tol || mx < -tol) continue;
                    touched[(size_t)(iy - iy0) * w + (ix - ix0)] = 1;
                    hits.emplace_back((uint32_t)((size_t)iy * N.nx + ix), (int32_t)i);
                }
        }
        std::sort(hits.begin(), hits.end());
        for (size_t a = 0; a < hits.size();) { // one candidate per touched cell: its edges + a reference point off the boundary
            size_t b = a;
            while (b < hits.size() && hits[b].first == hits[a].first) ++b;
            const uint32_t cell = hits[a].first;
            const int ix = (int)(cell % (uint32_t)N.nx), iy = (int)(cell / (uint32_t)N.nx);
            sg::RoadCand cd{};
            cd.poly = (int32_t)gq;
            cd.edge_off = (uint32_t)edge_lists.size();
            if (b - a > 65535) return -1;
            cd.n_edges = (uint16_t)(b - a);
            int loc = 2;
            for (int sel = 0; sel < RN_NREF && loc == 2; ++sel) {
                double rx, ry;
                sg::rn_ref_point(N, ix, iy, sel, rx, ry);
                loc = sg::rn_polygon_locate(B.edges.data(), e0, e1, rx, ry);
                cd.ref_sel = (uint8_t)sel;
            }
            if (loc == 2) return -2; // every reference point of the cell lies on this polygon's boundary
            cd.ref_inside = (uint8_t)(loc == 1);
            for (size_t k = a; k < b; ++k) edge_lists.push_back(hits[k].second);
            cells[cell] |= (uint16_t)(L << 8);
            (L ? entries : xentries).push_back({cell, cd});
            a = b;
        }
        for (int iy = iy0; iy <= iy1; ++iy) {
            bool known = false, inside = false;
            for (int ix = ix0; ix <= ix1; ++ix) {
                const uint32_t cell = (uint32_t)((size_t)iy * N.nx + ix);
                if (touched[(size_t)(iy - iy0) * w + (ix - ix0)]) {
                    known = false;
                } else {
                    if (!known) {
                        inside = sg::rn_polygon_locate(B.edges.data(), e0, e1, N.x0 + (ix + 0.5) * c, N.y0 + (iy + 0.5) * c) == 1;
                        known = true;
                    }
                    if (inside) {
                        cells[cell] |= (uint16_t)L;
                        grefs.push_back({cell, (int32_t)gq, (uint32_t)sg::RG_FULL << sg::RG_SHIFT | (uint32_t)gq});
                    }
                }
            }
        }
    }
    std::stable_sort(entries.begin(), entries.end(), [](const Entry &x, const Entry &y) { return x.cell < y.cell; });
    std::stable_sort(xentries.begin(), xentries.end(), [](const Entry &x, const Entry &y) { return x.cell < y.cell; });
    // CSR (global over all networks: cell_off has one entry per cell + a final one appended by the caller)
    size_t k = 0, kx = 0;
    for (size_t cell = 0; cell < ncell; ++cell) {
        B.cell_off.push_back((uint32_t)B.cand.size());
        while (k < entries.size() && entries[k].cell == cell) {
            grefs.push_back({(uint32_t)cell, entries[k].cd.poly, (uint32_t)sg::RG_CAND << sg::RG_SHIFT | (uint32_t)B.cand.size()});
            B.cand.push_back(entries[k++].cd);
        }
        while (kx < xentries.size() && xentries[kx].cell == cell) {
            grefs.push_back({(uint32_t)cell, xentries[kx].cd.poly, (uint32_t)sg::RG_XCAND << sg::RG_SHIFT | (uint32_t)B.xcand.size()});
            B.xcand.push_back(xentries[kx++].cd);
        }
    }
    if (std::max(B.cand.size(), std::max(B.xcand.size(), B.poly_layers.size())) >= ((size_t)1 << sg::RG_SHIFT)) return -3;
    if (B.ref.size() + grefs.size() >= ((size_t)1 << 32)) return -3;
    // a polygon is in a cell's list once: as a candidate where its boundary touches the cell, else as a cover
    std::sort(grefs.begin(), grefs.end(), [](const GRef &x, const GRef &y) { return x.cell != y.cell ? x.cell < y.cell : x.poly < y.poly; });
    size_t kg = 0;
    for (size_t cell = 0; cell < ncell; ++cell) {
        B.ref_off.push_back((uint32_t)B.ref.size());
        while (kg < grefs.size() && grefs[kg].cell == cell) B.ref.push_back(grefs[kg++].code);
    }
    B.nets.push_back(N);
    return 0;
}
} // namespace

extern "C" int sg_set_road_networks(sg_handle *h, const sg_road_networks *in)
{
    if (!h || !in) return h ? fail(h, SG_ERR_INVALID, "sg_set_road_networks: null argument") : SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_set_road_networks: no scenarios uploaded");
    if (in->n_networks < 0 || !in->net_of_scenario || (in->n_networks > 0 && (!in->poly_off || !in->ring_off || !in->vert_off || !in->layers)))
        return fail(h, SG_ERR_INVALID, "sg_set_road_networks: null array");
    for (int r = 0; r < h->R; ++r)
        if (in->net_of_scenario[r] < -1 || in->net_of_scenario[r] >= in->n_networks)
            return fail(h, SG_ERR_INVALID, "sg_set_road_networks: net_of_scenario[%d]=%d out of range", r, in->net_of_scenario[r]);
    const int64_t n_poly = in->n_networks ? in->poly_off[in->n_networks] : 0;
    for (int n = 0; n < in->n_networks; ++n)
        if (in->poly_off[n + 1] < in->poly_off[n] || in->poly_off[0] != 0) return fail(h, SG_ERR_INVALID, "sg_set_road_networks: poly_off not monotone");
    for (int64_t q = 0; q < n_poly; ++q) {
        if (in->ring_off[q + 1] < in->ring_off[q] || in->ring_off[0] != 0) return fail(h, SG_ERR_INVALID, "sg_set_road_networks: ring_off not monotone");
        for (int64_t r = in->ring_off[q]; r < in->ring_off[q + 1]; ++r)
            if (in->vert_off[r + 1] < in->vert_off[r] || in->vert_off[0] != 0) return fail(h, SG_ERR_INVALID, "sg_set_road_networks: vert_off not monotone");
    }
    const int64_t n_vert = n_poly ? in->vert_off[in->ring_off[n_poly]] : 0;
    if (n_vert > 0 && !in->verts) return fail(h, SG_ERR_INVALID, "sg_set_road_networks: null verts");
    for (int64_t i = 0; i < 2 * n_vert; ++i)
        if (!std::isfinite(in->verts[i])) return fail(h, SG_ERR_INVALID, "sg_set_road_networks: vertex %lld is not finite", (long long)(i / 2));
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_pool(h->road_allocs);
    forget_lanes(h); // (they index these networks)
    h->has_road = false;
    h->p.road = nullptr;
    h->geom = sg::RoadGeom{};
    RoadBuild B;
    B.poly_edge_off.push_back(0);
    B.imp_off.push_back(0);
    for (int n = 0; n < in->n_networks; ++n)
        if (int brc = build_road_network(in, n, B))
            return fail(h, SG_ERR_INVALID, "sg_set_road_networks: network %d cannot be indexed (%s)", n,
                        brc == -1 ? "more than 65535 edges of one polygon in one cell"
                        : brc == -3 ? "more than 2^30 polygons or boundary cells" : "a cell whose reference points all lie on a polygon boundary");
    B.cell_off.push_back((uint32_t)B.cand.size());
    B.ref_off.push_back((uint32_t)B.ref.size());
    if (B.ref.empty()) B.ref.push_back(0u);
    if (B.xcand.empty()) B.xcand.push_back(sg::RoadCand{});
    if (B.xcand_edges.empty()) B.xcand_edges.push_back(0);
    if (B.cand.empty()) B.cand.push_back(sg::RoadCand{});
    if (B.cand_edges.empty()) B.cand_edges.push_back(0);
    if (B.edges.empty()) B.edges.assign(4, 0.0);
    if (B.nets.empty()) { B.nets.push_back(sg::RoadNet{0.0, 0.0, 1.0, 1, 1, 0}); B.cells.push_back(0); B.cell_off.insert(B.cell_off.begin(), 0u); B.ref_off.insert(B.ref_off.begin(), 0u); B.poly0.push_back(0); B.net_flags.push_back(0); B.imp_off.push_back(0); }
    if (B.imp_edges.empty()) B.imp_edges.assign(4, 0.0);
    std::vector<int32_t> nos(in->net_of_scenario, in->net_of_scenario + h->R);
    auto &A = h->road_allocs;
    sg::RoadIndex R{};
    int rc = 0;
    if ((rc = dev_upload(h, A, &R.nets, B.nets))) return rc;
    if ((rc = dev_upload(h, A, &R.net_of_scen, nos))) return rc;
    if ((rc = dev_upload(h, A, &R.cells, B.cells))) return rc;
    if ((rc = dev_upload(h, A, &R.cell_off, B.cell_off))) return rc;
    if ((rc = dev_upload(h, A, &R.cand, B.cand))) return rc;
    if ((rc = dev_upload(h, A, &R.cand_edges, B.cand_edges))) return rc;
    if ((rc = dev_upload(h, A, &R.edges, B.edges))) return rc;
    if ((rc = dev_upload(h, A, &R.poly_layers, B.poly_layers))) return rc;
    if ((rc = dev_upload(h, A, &R.net_flags, B.net_flags))) return rc;
    if ((rc = dev_upload(h, A, &R.imp_off, B.imp_off))) return rc;
    if ((rc = dev_upload(h, A, &R.imp_edges, B.imp_edges))) return rc;
    {   // the filter tables of ped_boundary_terms (sgym_road.hpp)
        const size_t ne = B.imp_edges.size() / 4;
        std::vector<double> aux(ne * 4, 0.0), big(B.imp_off.size() - 1, 0.0);
        for (size_t i = 0; i < ne; ++i) {
            const double *e = &B.imp_edges[i * 4];
            const double dx = e[2] - e[0], dy = e[3] - e[1];
            aux[i * 4] = dx;
            aux[i * 4 + 1] = dy;
            aux[i * 4 + 2] = 1.0 / (dx * dx + dy * dy); // (a point edge: inf -- the filter's clamp turns the NaN it makes into t = 0)
        }
        for (size_t n = 0; n + 1 < B.imp_off.size(); ++n)
            for (int64_t i = B.imp_off[n] * 4; i < B.imp_off[n + 1] * 4; ++i) big[n] = std::max(big[n], std::fabs(B.imp_edges[(size_t)i]));
        if (big.empty()) big.push_back(0.0);
        if ((rc = dev_upload(h, A, &R.imp_aux, aux))) return rc;
        if ((rc = dev_upload(h, A, &R.imp_m, big))) return rc;
    }
    sg::RoadGeom G{};
    if ((rc = dev_upload(h, A, &G.ref_off, B.ref_off))) return rc;
    if ((rc = dev_upload(h, A, &G.ref, B.ref))) return rc;
    if ((rc = dev_upload(h, A, &G.xcand, B.xcand))) return rc;
    if ((rc = dev_upload(h, A, &G.xcand_edges, B.xcand_edges))) return rc;
    if ((rc = dev_upload(h, A, &G.poly0, B.poly0))) return rc;
    R.n_nets = in->n_networks;
    std::vector<sg::RoadIndex> one(1, R);
    const sg::RoadIndex *dR = nullptr;
    if ((rc = dev_upload(h, A, &dR, one))) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // host vectors go out of scope
    h->road = R;
    h->geom = G;
    h->p.road = dR;
    h->has_road = true;
    ++h->generation;
    return SG_OK;
}

// ---- lane centre lines (lane_observation_kernel, sgym_observers.hpp) --------------------------------------------------
// One device row per centre-line segment, lane by lane in point order, built by append_segments (sgym_host.hpp).  This unit is
// compiled with -ffp-contract=off like the rest of the library: its products and sums are the unfused ones the definition in
// include/sgym.h names.
extern "C" int sg_set_lanes(sg_handle *h, const sg_lanes *in)
{
    if (!h || !in) return h ? fail(h, SG_ERR_INVALID, "sg_set_lanes: null argument") : SG_ERR_INVALID;
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_set_lanes: no scenarios uploaded");
    if (!h->has_road) return fail(h, SG_ERR_STATE, "sg_set_lanes: no road networks set (sg_set_road_networks comes first)");
    if (in->n_networks != h->road.n_nets)
        return fail(h, SG_ERR_INVALID, "sg_set_lanes: %d networks, sg_set_road_networks got %d", in->n_networks, h->road.n_nets);
    const int nn = in->n_networks;
    if (nn > 0 && !in->lane_off) return fail(h, SG_ERR_INVALID, "sg_set_lanes: null lane_off");
    for (int n = 0; n < nn; ++n)
        if (in->lane_off[0] != 0 || in->lane_off[n + 1] < in->lane_off[n]) return fail(h, SG_ERR_INVALID, "sg_set_lanes: lane_off not monotone");
    const int64_t n_lanes = nn ? in->lane_off[nn] : 0;
    if (n_lanes > 0 && (!in->pt_off || !in->succ_off)) return fail(h, SG_ERR_INVALID, "sg_set_lanes: null pt_off or succ_off");
    if (n_lanes >= 0x7fffffffLL) return fail(h, SG_ERR_INVALID, "sg_set_lanes: 2^31 - 1 or more lanes");
    for (int64_t q = 0; q < n_lanes; ++q) {
        if (in->pt_off[0] != 0 || in->pt_off[q + 1] < in->pt_off[q]) return fail(h, SG_ERR_INVALID, "sg_set_lanes: pt_off not monotone");
        if (in->succ_off[0] != 0 || in->succ_off[q + 1] < in->succ_off[q]) return fail(h, SG_ERR_INVALID, "sg_set_lanes: succ_off not monotone");
    }
    const int64_t n_pts = n_lanes ? in->pt_off[n_lanes] : 0, n_succ = n_lanes ? in->succ_off[n_lanes] : 0;
    if ((n_pts > 0 && !in->pts) || (n_succ > 0 && !in->succ)) return fail(h, SG_ERR_INVALID, "sg_set_lanes: null pts or succ");
    if (n_pts >= 0x7fffffffLL || n_succ >= 0x7fffffffLL) return fail(h, SG_ERR_INVALID, "sg_set_lanes: 2^31 - 1 or more points or successors");
    for (int n = 0; n < nn; ++n) {
        const int64_t in_net = in->lane_off[n + 1] - in->lane_off[n];
        for (int64_t m = in->succ_off[in->lane_off[n]]; m < in->succ_off[in->lane_off[n + 1]]; ++m)
            if (in->succ[m] < 0 || in->succ[m] >= in_net)
                return fail(h, SG_ERR_INVALID, "sg_set_lanes: succ[%lld]=%d outside the %lld lanes of network %d", (long long)m, in->succ[m], (long long)in_net, n);
    }
    std::vector<sg::LaneSeg> segs;
    std::vector<sg::LaneRow> rows((size_t)n_lanes);
    std::vector<sg::LaneNet> nets((size_t)nn);
    std::vector<int32_t> succ;
    for (int n = 0; n < nn; ++n) {
        const int64_t l0 = in->lane_off[n], l1 = in->lane_off[n + 1];
        nets[(size_t)n].lane0 = (int32_t)l0; nets[(size_t)n].lane1 = (int32_t)l1;
        nets[(size_t)n].seg0 = (int32_t)segs.size();
        for (int64_t q = l0; q < l1; ++q) {
            sg::LaneRow &row = rows[(size_t)q];
            row.seg0 = (int32_t)segs.size();
            row.total = append_segments(segs, in->pts, in->pt_off[q], in->pt_off[q + 1], (int32_t)q, row.seg0);
            row.seg1 = (int32_t)segs.size();
            row.succ0 = (int32_t)succ.size();
            for (int64_t m = in->succ_off[q]; m < in->succ_off[q + 1]; ++m) succ.push_back((int32_t)(l0 + in->succ[m]));
            std::sort(succ.begin() + row.succ0, succ.end()); // ascending, each once: "the lowest-index successor" is the first that has segments
            succ.erase(std::unique(succ.begin() + row.succ0, succ.end()), succ.end());
            row.succ1 = (int32_t)succ.size();
        }
        nets[(size_t)n].seg1 = (int32_t)segs.size();
    }
    if (segs.size() >= (size_t)0x7fffffff) return fail(h, SG_ERR_INVALID, "sg_set_lanes: 2^31 - 1 or more segments");
    if (segs.empty()) segs.push_back(sg::LaneSeg{}); // (seg != nullptr says that lanes are set)
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // (a queued sg_lane_observation may still read the previous lanes)
    forget_lanes(h);
    auto &A = h->lane_allocs;
    sg::LaneIndex L{};
    int rc = 0;
    if (!(rc = dev_upload(h, A, &L.seg, segs)) && !(rc = dev_upload(h, A, &L.lane, rows)) && !(rc = dev_upload(h, A, &L.succ, succ)))
        rc = dev_upload(h, A, &L.net, nets);
    if (rc) { forget_lanes(h); return rc; }
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // host vectors go out of scope
    L.net_of_scen = h->road.net_of_scen;
    h->lanes = L;
    return SG_OK;
}

// ---- which road geometries contain each entity / each point (sgym_geom.hpp) ------------------------------------------
// n queries on the handle's stream (behind whatever rollout work is pending there) with HOST outputs, through a scratch of their own
// (h->road_info; scratch(), sgym_host.hpp) as
// [count][layers][geoms]; scen / xy: the n points on the host, which go into the scratch behind the outputs' room -- [n][2]
// doubles, then [n] scenarios -- in front of the kernel (nullptr: the entity slots)
static int road_info_host(sg_handle *h, const char *who, int64_t n, const int32_t *scen, const double *xy, int32_t cap, int32_t *count,
                          int32_t *geoms, uint32_t *layers)
{
    const size_t nb = (size_t)n * 4;
    return deliver(h, who, false, h->road_info, {{count, nb}, {layers, nb}, {geoms, nb * cap}}, xy ? nb * 5 : 0, [&](void *const *d) {
        double *const d_xy = static_cast<double *>(d[3]);
        int32_t *const d_scen = xy ? reinterpret_cast<int32_t *>(d_xy + 2 * n) : nullptr;
        if (xy) {
            hipError_t e = hipMemcpyAsync(d_xy, xy, nb * 4, hipMemcpyHostToDevice, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(d_scen, scen, nb, hipMemcpyHostToDevice, h->stream);
            if (e != hipSuccess) return e;
        }
        sgl::road_info(h->stream, h->p, h->road, h->geom, h->has_road, d_scen, d_xy, n, cap, static_cast<int32_t *>(d[0]), static_cast<int32_t *>(d[2]),
                       static_cast<uint32_t *>(d[1]));
        return hipGetLastError();
    });
}

extern "C" int sg_road_info(sg_handle *h, int32_t cap, int32_t *count, int32_t *geoms, uint32_t *layers, int32_t outputs_device)
{
    if (!h) return SG_ERR_INVALID;
    if (!geoms) cap = 0;
    if (!count || cap < 0) return fail(h, SG_ERR_INVALID, "sg_road_info: null count or cap < 0");
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_road_info: no scenarios uploaded");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int64_t n = (int64_t)h->R * h->E;
    if (outputs_device) { // stream-ordered, not synchronised (sg_raster_map_device)
        sgl::road_info(h->stream, h->p, h->road, h->geom, h->has_road, nullptr, nullptr, n, cap, count, geoms, layers);
        HIP_TRY(h, hipGetLastError());
        return SG_OK;
    }
    return road_info_host(h, "sg_road_info", n, nullptr, nullptr, cap, count, geoms, layers);
}

extern "C" int sg_road_info_points(sg_handle *h, int64_t n, const int32_t *scenario_of_point, const double *xy, int32_t cap, int32_t *count,
                                   int32_t *geoms, uint32_t *layers)
{
    if (!h) return SG_ERR_INVALID;
    if (!geoms) cap = 0;
    if (n < 0 || !count || cap < 0 || (n > 0 && (!xy || !scenario_of_point))) return fail(h, SG_ERR_INVALID, "sg_road_info_points: null array, n < 0 or cap < 0");
    if (!h->uploaded) return fail(h, SG_ERR_STATE, "sg_road_info_points: no scenarios uploaded");
    for (int64_t i = 0; i < n; ++i)
        if (scenario_of_point[i] < 0 || scenario_of_point[i] >= h->R)
            return fail(h, SG_ERR_INVALID, "sg_road_info_points: scenario_of_point[%lld]=%d out of range", (long long)i, scenario_of_point[i]);
    if (n == 0) return SG_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return road_info_host(h, "sg_road_info_points", n, scenario_of_point, xy, cap, count, geoms, layers);
}
