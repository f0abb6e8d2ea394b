"""The exact reference for "which polygons contain this point" and the adversarial road networks and query points that
tests/test_road_index_adversarial.py aims at the device's cell index (build_road_network in csrc/h_road.hip, rn_* in
csrc/sgym_road.hpp and sgym_geom.hpp).  A plain module, like standin_engine.py.

The rule (README N6): a point is in a polygon iff it lies strictly inside its rings by the crossing number (ray
towards +x, half-open in y, rings as given, even-odd); a point ON a ring is in nothing.  Here it is decided with exact
rational arithmetic (fractions.Fraction) wherever an fp64 filter cannot decide -- no text shared with the oracle's or the
device's orientation predicate.  Degenerate rings (fewer than three vertices, zero area, repeated vertices, first vertex
repeated at the end) need no case of their own: their edges are edges like any others."""
from fractions import Fraction

import numpy as np

# rn_ref_point (scenario_gym_amd/csrc/sgym_road.hpp, arrays FX / FY): the eight candidate reference points of a cell, as
# fractions of the cell side.  Quoted to AIM polygons and points at them; no expected answer depends on it.
REF_FX = (0.5, 0.25, 0.75, 0.25, 0.75, 0.375, 0.625, 0.4375)
REF_FY = (0.5, 0.25, 0.25, 0.75, 0.75, 0.5625, 0.3125, 0.6875)

PLACEMENTS = ((0.0, 0.0), (12345.678, -9876.543), (4.5e5, 5.4e6), (-3.2e6, 7.1e6), (2.0 ** 40, -2.0 ** 40))
LAYER_MIX = (3, 0, 9, 48, 5, 80, 128, 0, 1, 16, 2, 64)  # SG_LAYER_* bits, some polygons without any


# ---------------------------------------------------------------------------------------------------- the exact reference
def _exact_orient(ax, ay, bx, by, px, py):
    F = Fraction
    return (F(bx) - F(ax)) * (F(py) - F(ay)) - (F(by) - F(ay)) * (F(px) - F(ax))


def _contains_many(edges, poly_edge_off, px, py, with_on=False):
    """bool [n points][n polygons]; see _contains_all.  Points that are not finite, beyond 1e100 or outside the box of all vertices are in
    nothing (and never reach the arithmetic).  with_on: also bool [n points][n polygons], the point lies ON a ring of it."""
    px, py = np.asarray(px, np.float64).ravel(), np.asarray(py, np.float64).ravel()
    off = np.asarray(poly_edge_off, np.int64)
    out = np.zeros((len(px), len(off) - 1), bool)
    on_ring = np.zeros_like(out)
    if len(edges) == 0 or len(px) == 0:
        return (out, on_ring) if with_on else out
    x1, y1, x2, y2 = (c[None, :] for c in np.asarray(edges, np.float64).T)
    near = np.isfinite(px) & np.isfinite(py) & (np.maximum(np.abs(px), np.abs(py)) < 1e100)
    if len(px) > 8:  # (many points: those outside the box of all vertices need no arithmetic)
        near &= (px >= min(x1.min(), x2.min())) & (px <= max(x1.max(), x2.max())) & (py >= min(y1.min(), y2.min())) & (py <= max(y1.max(), y2.max()))
    idx = np.nonzero(near)[0]
    step = max(1, 2_000_000 // edges.shape[0])
    for a in range(0, len(idx), step):
        sel = idx[a:a + step]
        qx, qy = px[sel, None], py[sel, None]
        o = (x2 - x1) * (qy - y1) - (y2 - y1) * (qx - x1)
        mag = np.abs((x2 - x1) * (qy - y1)) + np.abs((y2 - y1) * (qx - x1))
        box = (np.minimum(x1, x2) <= qx) & (qx <= np.maximum(x1, x2)) & (np.minimum(y1, y2) <= qy) & (qy <= np.maximum(y1, y2))
        straddle = (y1 > qy) != (y2 > qy)
        sign = np.sign(o)
        for i, k in zip(*np.nonzero((np.abs(o) <= 1e-9 * mag) & (straddle | box))):
            e = _exact_orient(x1[0, k], y1[0, k], x2[0, k], y2[0, k], qx[i, 0], qy[i, 0])
            sign[i, k] = (e > 0) - (e < 0)
        on = box & (sign == 0)
        cross = straddle & (np.where(y2 > y1, sign, -sign) > 0)
        zero = np.zeros((len(sel), 1), np.int64)
        n_cross = np.concatenate([zero, np.cumsum(cross, axis=1)], axis=1)
        n_on = np.concatenate([zero, np.cumsum(on, axis=1)], axis=1)
        n_cross, n_on = n_cross[:, off[1:]] - n_cross[:, off[:-1]], n_on[:, off[1:]] - n_on[:, off[:-1]]
        out[sel] = (n_cross % 2 == 1) & (n_on == 0)
        on_ring[sel] = n_on > 0
    return (out, on_ring) if with_on else out


def _contains_all(edges, poly_edge_off, px, py):
    """bool per polygon: crossing number of its rings for the ray towards +x, half-open in y; the orientation in exact rational
    arithmetic wherever fp64 could be in doubt; a point on an edge is in nothing."""
    return _contains_many(edges, poly_edge_off, [px], [py])[0]


def _edges_of(a):
    """([n][4] ring edges polygon by polygon, edge offsets per polygon) of a polygon_arrays() dict."""
    verts = np.asarray(a["verts"], np.float64).reshape(-1, 2)
    edges, off = [np.zeros((0, 4))], [0]
    for q in range(len(a["ring_off"]) - 1):
        n = 0
        for r in range(a["ring_off"][q], a["ring_off"][q + 1]):
            v = verts[a["vert_off"][r]:a["vert_off"][r + 1]]
            edges.append(np.concatenate([v, np.roll(v, -1, axis=0)], axis=1))
            n += len(v)
        off.append(off[-1] + n)
    return np.concatenate(edges), np.array(off)


def contains_exact(arrays, px, py):
    """bool [n_polygons]: the polygons of a polygon_arrays() dict that contain the point (px, py)."""
    return _contains_all(*_edges_of(arrays), px, py)


def contains_exact_many(arrays, pts, with_on=False):
    """bool [n points][n_polygons] for points [n][2] (with_on: and the same for "on a ring of the polygon")."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    return _contains_many(*_edges_of(arrays), pts[:, 0], pts[:, 1], with_on)


# ---------------------------------------------------------------------------------------------------- networks
class _Net:
    """Polygons (lists of rings) collected into a polygon_arrays()-style dict; layer bits cycle through LAYER_MIX."""

    def __init__(self):
        self.polys = []

    def add(self, *rings, layer=None):
        self.polys.append(([np.asarray(r, np.float64).reshape(-1, 2) for r in rings], LAYER_MIX[len(self.polys) % len(LAYER_MIX)] if layer is None else layer))
        return self

    def arrays(self, offset=(0.0, 0.0), scale=1.0):
        """Vertices * scale + offset, rounded to fp64 once: what device and reference both read."""
        rings = [r for p, _ in self.polys for r in p]
        verts = np.concatenate(rings + [np.zeros((0, 2))]) * scale + np.asarray(offset, np.float64)
        return dict(ring_off=np.concatenate([[0], np.cumsum([len(p) for p, _ in self.polys])]).astype(np.int64),
                    vert_off=np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64),
                    verts=np.ascontiguousarray(verts), layers=np.array([l for _, l in self.polys], np.uint32))


def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _star(rng, cx, cy, r, m):
    ang = np.sort(rng.uniform(0, 2 * np.pi, m))
    rad = r * rng.uniform(0.55, 1.0, m)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)


def _comb(x0, y0, teeth, w, h):
    """Base of height w, `teeth` teeth of width w and height h, gaps of width w."""
    pts = [(x0, y0), (x0 + 2 * teeth * w - w, y0)]
    for t in reversed(range(teeth)):
        a = x0 + 2 * t * w
        pts += [(a + w, y0 + w + h), (a, y0 + w + h)] if t == teeth - 1 else [(a + w, y0 + w), (a + w, y0 + w + h), (a, y0 + w + h)]
        if t:
            pts.append((a, y0 + w))
    return pts


def _lattice_net(rng):
    n = _Net()
    n.add(_rect(0, 0, 3, 2)).add(_rect(4.5, 0.5, 7.5, 2.5)).add(_rect(10, 0, 11, 1)).add(_rect(12.5, 0.5, 13.5, 1.5))
    n.add([(0, 4), (4, 4), (4, 6), (2, 6), (2, 9), (0, 9)])                      # L
    n.add([(6.5, 4.5), (9.5, 4.5), (9.5, 5.5), (7.5, 5.5), (7.5, 8.5), (6.5, 8.5)])  # L on cell centres
    n.add(_comb(0, 12, 5, 1.0, 3.0)).add(_comb(12, 12, 6, 0.5, 2.5))
    for i in range(40):  # nested squares: 40 polygons contain the centre (the default cap is 32)
        h = 0.5 * (i + 1)
        n.add(_rect(30 - h, 30 - h, 30 + h, 30 + h))
    for _ in range(8):
        a, b = rng.integers(0, 40, 2) / 2 + (14, 0)
        w, h = rng.integers(1, 8, 2) / 2
        n.add(_rect(a, b, a + w, b + h))
    return n


def lattice(rng, offset=(0.0, 0.0)):
    """Axis-parallel shapes with integer and half-integer vertices: edges on cell lines, vertices on cell corners and centres."""
    return [_lattice_net(rng).arrays(offset)]


def trap_ring(k, ix, iy, origin=(0.0, 0.0), c=1.0):
    """A simple ring through the first k reference points of cell (ix, iy) (cell side c, cell lines on multiples of c from
    `origin`): they form a chain monotone in x, closed two cells below the cell."""
    pts = sorted((ix + REF_FX[s], iy + REF_FY[s]) for s in range(k))
    ring = pts + [(ix + 1.53125, iy - 2.03125), (ix - 0.59375, iy - 2.03125)]
    return np.asarray(ring) * c + np.asarray(origin, np.float64)


def trap_cells():
    return {k: (10 * k, 3) for k in range(1, 9)}


def traps(rng, offset=(0.0, 0.0), upto=7):
    """For k = 1..upto one polygon whose ring has the first k reference points of its cell (trap_cells()) as vertices: the
    builder has to fall back to reference point k.  upto = 8: no reference point is left -- the network must be refused.
    Cell lines stay on the integers: the translation is by floor(offset)."""
    n = _Net()
    origin = np.floor(np.asarray(offset, np.float64))
    for k in range(1, upto + 1):
        n.add(trap_ring(k, *trap_cells()[k], origin=origin))
    n.add(_rect(*(origin + (-2, -2)), *(origin + (95, 8))), layer=0)  # one polygon around them all
    return [n.arrays()]


def circle(nv, offset=(0.0, 0.0)):
    """A circle of radius 0.1 m with nv vertices inside one cell."""
    t = 2 * np.pi * np.arange(nv) / nv
    return _Net().add(np.stack([0.5 + 0.1 * np.cos(t), 0.5 + 0.1 * np.sin(t)], 1), layer=1).arrays(offset)


def thin(rng, offset=(0.0, 0.0)):
    """Slivers 1e-7 and 1e-3 m wide across many cells, 1 cm triangles, a spiral and a zig-zag with tens of edges per cell; and
    the largest polygon one cell can take (60,000 vertices; sg_road_networks allows 65,535 edges of one polygon per cell)."""
    n = _Net()
    n.add([(0, 0), (20, 13), (20, 13 + 1e-7), (0, 1e-7)]).add([(0, 5), (25, 17), (25, 17.001), (0, 5.001)])
    n.add([(0.25, 20), (19.75, 20.5), (19.75, 20.5 + 1e-7)])
    for _ in range(6):
        x, y = rng.integers(0, 20, 2) + rng.uniform(0.1, 0.8, 2)
        n.add([(x, y), (x + 0.01, y), (x, y + 0.01)])
    t = np.linspace(0.0, 6 * np.pi, 420)
    r0, r1 = 0.4 + 0.14 * t, 0.5 + 0.14 * t
    n.add(np.concatenate([np.stack([40 + r0 * np.cos(t), 10 + r0 * np.sin(t)], 1), np.stack([40 + r1 * np.cos(t), 10 + r1 * np.sin(t)], 1)[::-1]]))
    i = np.arange(241)
    n.add(np.concatenate([np.stack([30 + i * 0.05, 30 + (i % 2) * 0.8 + 0.01 * rng.random(241)], 1), [(42, 29.5), (30, 29.5)]]))
    return [n.arrays(offset), circle(60000, offset)]


def holes(rng, offset=(0.0, 0.0)):
    """Several holes, a hole touching its exterior ring in one vertex, an island inside a hole, a hole wider than several cells."""
    n = _Net()
    n.add(_rect(0, 0, 20, 20), _rect(2, 2, 4, 4)[::-1], _rect(6.5, 6.5, 8, 9)[::-1], _rect(10, 2, 18, 8)[::-1], _rect(3.25, 12.125, 3.75, 12.875))
    n.add(_rect(12, 4, 14, 6)).add(_rect(12.5, 4.5, 13.5, 5.5), layer=0)                # islands in the wide hole
    n.add(_rect(30, 0, 40, 10), [(30, 0), (34, 2), (32, 4)])                               # hole touching a vertex of the exterior
    n.add(_rect(30, 12, 40, 22), [(30, 17), (33, 15), (33, 19)])                           # ... and touching an edge of it
    ext, hole = _star(rng, 60, 12, 11, 40), _star(rng, 60, 12, 5, 17)
    n.add(ext, hole[::-1]).add(_star(rng, 60, 12, 2.5, 9))
    n.add(_rect(0, 30, 30, 50), *[_star(rng, 3 + 4 * j, 34 + 6 * (j % 3), 1.4, 7) for j in range(7)])
    return [n.arrays(offset)]


def degenerate(rng, offset=(0.0, 0.0)):
    """Rings of two vertices, collinear rings, repeated vertices, closed rings (first = last), polygons without rings and rings
    without vertices; an empty network; a network of one point-sized ring."""
    n = _Net()
    n.add([(1, 1), (4, 3)]).add([(0, 5), (2, 6), (6, 8)]).add([(8, 0), (8, 0), (11, 0), (11, 3), (11, 3), (11, 3), (8, 3)])
    n.add(_rect(0, 10, 4, 13) + [(0, 10)]).add(_rect(6, 10, 12, 14), [(7, 11), (10, 13)], [(8, 12), (8, 12), (8, 12)])
    n.add().add(np.zeros((0, 2)), _rect(14, 0, 17, 2)).add([(15.5, 1.0)]).add([(2.5, 11.5)] * 3)
    n.add(_rect(20, 0, 24, 4), _rect(20, 0, 24, 4))                   # a hole equal to the exterior: nothing inside
    n.add([(20, 6), (24, 6), (24, 10), (20, 10), (20, 6), (24, 6), (24, 10), (20, 10)])  # the same ring walked twice
    n.add([(0, 16), (6, 16), (0, 20), (6, 20)])                        # a bow tie
    empty = _Net().arrays()
    return [n.arrays(offset), empty, _Net().add([(0.3, 0.7)]).arrays(offset)]


def stars(rng, offset=(0.0, 0.0), scale=1.0):
    n = _Net()
    for _ in range(10):
        n.add(_star(rng, *rng.uniform(-40, 40, 2), rng.uniform(8, 40), int(rng.integers(5, 60))))
    return [n.arrays(offset, scale)]


FAMILIES = dict(lattice=lattice, traps=traps, thin=thin, holes=holes, degenerate=degenerate, stars=stars)


def coarse(rng, name):
    """square1600 / square3200: networks 1.6 km and 3.2 km wide (the builder's cell side becomes 2 m and 4 m) holding the
    lattice and star families scaled up plus small shapes; strip: 100 km x 3 m (1 m cells, about 100,000 x 7 of them)."""
    n = _Net()
    if name == "strip":
        n.add(_rect(0, 0, 100000, 3), layer=1).add([(10, 1), (90000, 2), (90000, 2.001), (10, 1.001)], layer=16)
        for x in np.arange(0.0, 100000.0, 9999.5):
            n.add(_rect(x + 1, 0.5, x + 3, 2.5)).add([(x + 5.2, 1.2), (x + 5.21, 1.2), (x + 5.2, 1.21)])
        return [n.arrays()]
    side = dict(square1600=1600.0, square3200=3200.0)[name]
    s = side / 64
    lat = _lattice_net(rng)
    for rings, layer in lat.polys:
        n.add(*[r * s for r in rings], layer=layer)
    for _ in range(8):
        n.add(_star(rng, *rng.uniform(0.2 * side, 0.8 * side, 2), rng.uniform(0.05, 0.2) * side, int(rng.integers(5, 60))))
    for _ in range(12):
        x, y = np.floor(rng.uniform(0, side, 2)) + rng.uniform(0.1, 0.8, 2)
        n.add([(x, y), (x + 0.01, y), (x, y + 0.01)]).add(_rect(np.floor(x) + 3, np.floor(y), np.floor(x) + 4, np.floor(y) + 1))
    n.add(_rect(0, 0, 1, 1)).add(_rect(side - 1, side - 1, side, side))
    return [n.arrays()]


COARSE = ("square1600", "square3200", "strip")


# ---------------------------------------------------------------------------------------------------- query points
def grid_of(arrays):
    """(x0, y0, cell side, nx, ny) of the uniform grid build_road_network lays over a network (csrc/h_road.hip: 1 m cells,
    doubled while there would be more than 2^21; one cell of margin).  Restated to AIM points at cell lines; no expected answer
    depends on it."""
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 2)
    if len(v) == 0:
        return 0.0, 0.0, 1.0, 1, 1
    lo, hi = v.min(0), v.max(0)
    c = 1.0
    while ((hi[0] - lo[0]) / c + 4) * ((hi[1] - lo[1]) / c + 4) > 2097152.0:
        c *= 2
    x0, y0 = np.floor(lo / c) * c - c
    return float(x0), float(y0), c, int(np.ceil((hi[0] - x0) / c)) + 2, int(np.ceil((hi[1] - y0) / c)) + 2


CLASSES = ("uniform", "vertex", "midpoint", "on_axis_edge", "cell_line", "sixteenth", "through_vertex", "prolongation", "outside")
MAX_RING_SAMPLE = 128  # of a ring with more vertices than 2048 (the 60,000-vertex circle), this many seeded ones are aimed at


def _around(p):
    """Each point and its np.nextafter neighbours to both sides in x and in y."""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    return np.concatenate([p, np.stack([np.nextafter(x, -np.inf), y], 1), np.stack([np.nextafter(x, np.inf), y], 1),
                           np.stack([x, np.nextafter(y, -np.inf)], 1), np.stack([x, np.nextafter(y, np.inf)], 1)])


def adversarial_points(arrays, rng, n_uniform=6000):
    """(points [n][2], class index [n] into CLASSES) for one network: see the issue text quoted in each branch."""
    x0, y0, c, nx, ny = grid_of(arrays)
    verts = np.asarray(arrays["verts"], np.float64).reshape(-1, 2)
    vo = np.asarray(arrays["vert_off"])
    keep = []
    for r in range(len(vo) - 1):  # the vertices aimed at
        k = np.arange(vo[r], vo[r + 1])
        keep.append(k if len(k) <= 2048 else np.sort(rng.choice(k, MAX_RING_SAMPLE, replace=False)))
    keep = np.concatenate(keep + [np.zeros(0, np.int64)]).astype(np.int64)
    nxt = np.arange(len(verts)) + 1
    for r in range(len(vo) - 1):
        if vo[r + 1] > vo[r]:
            nxt[vo[r + 1] - 1] = vo[r]
    A, B = verts[keep], verts[nxt[keep]] if len(keep) else verts[keep]
    out = {}
    gx1, gy1 = x0 + nx * c, y0 + ny * c
    out["uniform"] = np.stack([rng.uniform(x0 - 2 * c, gx1 + 2 * c, n_uniform), rng.uniform(y0 - 2 * c, gy1 + 2 * c, n_uniform)], 1)
    out["vertex"] = _around(A)
    out["midpoint"] = 0.5 * (A + B)
    ax = (A[:, 0] == B[:, 0]) | (A[:, 1] == B[:, 1])
    t = np.concatenate([np.full(ax.sum(), 0.25), np.full(ax.sum(), 0.5), rng.random(ax.sum())])[:, None]
    Aa, Ba = np.tile(A[ax], (3, 1)), np.tile(B[ax], (3, 1))
    out["on_axis_edge"] = np.where(Aa == Ba, Aa, Aa + t * (Ba - Aa))  # (the shared coordinate stays exact)
    # cell lines and corners: multiples of the cell side (and of 1, 2, 4 m) around the cells that hold vertices and at random
    cells = np.unique(np.floor((A - (x0, y0)) / c), axis=0) if len(A) else np.zeros((0, 2))
    if len(cells) > 60:
        cells = cells[rng.choice(len(cells), 60, replace=False)]
    rand = np.stack([rng.integers(0, nx, 60), rng.integers(0, ny, 60)], 1).astype(np.float64)
    corners = []
    for s in sorted({1.0, 2.0, 4.0, c}):
        base = np.concatenate([cells, rand]) * c
        base = np.floor(base / s) * s
        for dx in (0.0, s):
            for dy in (0.0, s):
                corners.append(base + (dx, dy) + (x0, y0))
    corners = np.unique(np.concatenate(corners), axis=0)
    X, Y = corners[:, 0], corners[:, 1]
    xs = [np.nextafter(X, -np.inf), X, np.nextafter(X, np.inf)]
    ys = [np.nextafter(Y, -np.inf), Y, np.nextafter(Y, np.inf)]
    line = [np.stack([a, b], 1) for a in xs for b in ys]
    line += [np.stack([a, Y + c * rng.random(len(Y))], 1) for a in xs] + [np.stack([X + c * rng.random(len(X)), b], 1) for b in ys]
    out["cell_line"] = np.concatenate(line)
    # the c/16 lattice in cells that hold vertices (every reference point of rn_ref_point is on it)
    sub = cells[rng.choice(len(cells), 24, replace=False)] if len(cells) > 24 else cells
    u = np.arange(17) / 16.0
    lat = np.stack(np.meshgrid(u, u, indexing="ij"), -1).reshape(-1, 2)
    out["sixteenth"] = ((sub[:, None, :] + lat[None]) * c + (x0, y0)).reshape(-1, 2)
    # vertices V on the c/32 lattice: P = 2V - R for every reference point R of V's cell, where P stays in the cell -- the
    # segment R -> P passes exactly through V
    thr = []
    if len(A):
        f = (A - (x0, y0)) / c
        onl = (np.floor(f * 32) == f * 32).all(1)
        cell = np.floor(f[onl])
        for s in range(8):
            R = (cell + (REF_FX[s], REF_FY[s])) * c + (x0, y0)
            P = 2 * A[onl] - R
            thr.append(P[(np.floor((P - (x0, y0)) / c) == cell).all(1)])
    out["through_vertex"] = np.concatenate(thr + [np.zeros((0, 2))])
    out["prolongation"] = np.concatenate([B + t * (B - A) for t in (1.0, 0.5, 0.0009765625)] + [A - 1.0 * (B - A)])
    big = [x0 - 0.5 * c, gx1 + 0.5 * c, 1e15, -1e15, 1e300, -1e300, np.inf, -np.inf, np.nan, x0 + 0.5 * nx * c]
    bigy = [y0 - 0.5 * c, gy1 + 0.5 * c, 1e15, -1e15, 1e300, -1e300, np.inf, -np.inf, np.nan, y0 + 0.5 * ny * c]
    out["outside"] = np.array([(a, b) for i, a in enumerate(big) for j, b in enumerate(bigy) if not (i == 9 and j == 9)])
    pts = np.concatenate([out[k].reshape(-1, 2) for k in CLASSES])
    cls = np.concatenate([np.full(len(out[k]), i, np.int32) for i, k in enumerate(CLASSES)])
    return np.ascontiguousarray(pts), cls


N_NETWORKS = dict(thin=2, degenerate=3)  # networks per case (default 1)


def cases():
    """[(id, family or coarse name, placement index or None)]: everything the tests are parametrised over."""
    return [(f"{f}-p{p}", f, p) for f in FAMILIES for p in range(len(PLACEMENTS))] + [(n, n, None) for n in COARSE]


def networks_of(name, placement):
    """The networks of one case, seeded by the case alone."""
    rng = np.random.default_rng([17, sorted(list(FAMILIES) + list(COARSE)).index(name)])
    return coarse(rng, name) if placement is None else FAMILIES[name](rng, PLACEMENTS[placement])


def points_of(name, placement, nets):
    rng = np.random.default_rng([29, sorted(list(FAMILIES) + list(COARSE)).index(name), 0 if placement is None else placement + 1])
    return [adversarial_points(a, rng) for a in nets]
