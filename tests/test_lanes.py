"""Lane-frame vector observations (sg_set_lanes, sg_lane_observation, sg_lane_observation_observers): where the ego of every
scenario, or any observer of sg_set_observers, sits relative to the nearest lane centre lines of its scenario's road network,
and where those lines go next.  The reference has no such sensor (it only stores Lane.center and the successor ids), so the
yardstick is `lane_reference` below -- a numpy restatement of the definition in include/sgym.h over the poses and presence read
back through the state view, with the oracle's sin / cos.  Every comparison is bit for bit on the features and exact on lanes
and counts."""
import math
import os
import re

import numpy as np
import pytest

from conftest import load_golden, scenario_arrays
from test_host_api import scenario_from_arrays

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SG_ERR_INVALID, SG_ERR_STATE = -1, -3
INF = float("inf")
MAX_HOPS = 4
SIX_LANE, RURAL, SMALLEST = "dRisk Unity 6-lane Intersection", "Rural_Road_Network", "Greenwich_Road_Network_003"
# (lanes, centre points) of the committed networks
FIXTURE_COUNTS = {"Greenwich_Road_Network_002": (55, 4211), RURAL: (52, 7896), SMALLEST: (12, 564),
                  "Roundabout_Road_Network_001": (72, 5978), "Y_Intersection_Road_Network_001": (18, 1414), SIX_LANE: (132, 11040)}


@pytest.fixture
def sga():
    import scenario_gym_amd as sga

    return sga


# ---------------------------------------------------------------------------------------------------- the yardstick
class LaneTables:
    """The rows sg_set_lanes builds for one network, from lane_arrays()-style arrays: per segment a, b, e = b - a,
    L2 = ex*ex + ey*ey, len = sqrt(L2), cum (a sequential sum per lane), its lane; per lane the segment range, total and the
    successors (ascending, each once)."""

    def __init__(self, pt_off, pts, succ_off, succ):
        pts = np.asarray(pts, np.float64).reshape(-1, 2)
        self.n_lanes = len(pt_off) - 1
        a, b, self.seg_off = [], [], [0]
        for q in range(self.n_lanes):
            for i in range(int(pt_off[q]), int(pt_off[q + 1]) - 1):
                a.append(pts[i])
                b.append(pts[i + 1])
            self.seg_off.append(len(a))
        a, b = np.array(a, np.float64).reshape(-1, 2), np.array(b, np.float64).reshape(-1, 2)
        self.ax, self.ay, self.bx, self.by = a[:, 0].copy(), a[:, 1].copy(), b[:, 0].copy(), b[:, 1].copy()
        self.ex, self.ey = self.bx - self.ax, self.by - self.ay
        self.L2 = self.ex * self.ex + self.ey * self.ey
        self.len = np.sqrt(self.L2)
        self.cum, self.total = np.zeros(len(a)), np.zeros(self.n_lanes)
        for q in range(self.n_lanes):
            c = np.float64(0.0)
            for i in range(self.seg_off[q], self.seg_off[q + 1]):
                self.cum[i] = c
                c = c + self.len[i]
            self.total[q] = c  # = cum + len of the last segment
        self.succ = [sorted({int(z) for z in succ[int(succ_off[q]):int(succ_off[q + 1])]}) for q in range(self.n_lanes)]
        self._keys = {}

    def has_segments(self, q):
        return self.seg_off[q + 1] > self.seg_off[q]

    def keys(self, px, py):
        """Per lane that has a segment with a finite d2: (d2, lane, best segment), ascending; with the per-segment projection."""
        memo = self._keys.get((px, py))
        if memo is None:
            with np.errstate(all="ignore"):
                wx, wy = px - self.ax, py - self.ay
                t = (wx * self.ex + wy * self.ey) / self.L2
                at_a = (self.L2 == 0) | ~(t > 0)
                at_b = ~at_a & (t >= 1)
                cx = np.where(at_a, self.ax, np.where(at_b, self.bx, self.ax + t * self.ex))
                cy = np.where(at_a, self.ay, np.where(at_b, self.by, self.ay + t * self.ey))
                te = np.where(at_a, 0.0, np.where(at_b, 1.0, t))
                dx, dy = px - cx, py - cy
                d2 = dx * dx + dy * dy
            out = []
            for q in range(self.n_lanes):
                a, b = self.seg_off[q], self.seg_off[q + 1]
                finite = np.isfinite(d2[a:b])
                if finite.any():
                    best = a + int(np.argmin(np.where(finite, d2[a:b], np.inf)))  # (ties: the first, i.e. the lower segment index)
                    out.append((float(d2[best]), q, best))
            memo = self._keys[(px, py)] = (sorted(out), te, dx, dy)
        return memo

    def point_at(self, q, target):
        """The centre-line point at arclength `target` from the start of lane q, walked through the successors."""
        hops = 0
        while target > self.total[q] and hops < MAX_HOPS:
            nxt = next((z for z in self.succ[q] if self.has_segments(z)), None)
            if nxt is None:
                break
            target, q, hops = target - float(self.total[q]), nxt, hops + 1
        a, b = self.seg_off[q], self.seg_off[q + 1]
        if target > self.total[q]:
            return float(self.bx[b - 1]), float(self.by[b - 1])
        g = a + int(np.searchsorted(self.cum[a:b], target, side="right")) - 1  # the last segment with cum <= target
        u = (target - float(self.cum[g])) / float(self.len[g]) if self.len[g] != 0 else 0.0
        if u >= 1:
            return float(self.bx[g]), float(self.by[g])
        return float(self.ax[g]) + u * float(self.ex[g]), float(self.ay[g]) + u * float(self.ey[g])


def lane_reference(net, px, py, s, c, present, k, n_ahead, spacing, radius):
    """The definition for one observer: pose (px, py), (s, c) = sin, cos of its heading, against the LaneTables `net` (None:
    its scenario has no network).  Returns (feat [k, 6 + 2 * n_ahead], lanes [k], count).  Python floats are IEEE doubles and
    a * b + c * d is two products and a sum: nothing is fused."""
    feat, lanes = np.zeros((k, 6 + 2 * n_ahead)), np.full(k, -1, np.int32)
    if not present:
        return feat, lanes, -1
    if net is None:
        return feat, lanes, 0
    px, py, s, c, spacing = float(px), float(py), float(s), float(c), float(spacing)
    keys, te, dxs, dys = net.keys(px, py)
    r2 = np.float64(radius) * np.float64(radius)
    cands = [key for key in keys if key[0] <= r2]  # ascending (d2, lane index)
    for j, (d2, q, i) in enumerate(cands[:k]):
        ex, ey, ln, dx, dy = float(net.ex[i]), float(net.ey[i]), float(net.len[i]), float(dxs[i]), float(dys[i])
        ux, uy = (ex / ln, ey / ln) if ln != 0 else (0.0, 0.0)
        s0 = float(net.cum[i]) + float(te[i]) * ln
        row = [ux * dy - uy * dx, c * ux + s * uy, s * ux - c * uy, s0, float(net.total[q]) - s0, math.sqrt(d2)]
        for m in range(1, n_ahead + 1):
            x, y = net.point_at(q, s0 + float(m) * spacing)
            X, Y = x - px, y - py
            row += [X * c + Y * s, Y * c - X * s]
        feat[j], lanes[j] = row, q
    return feat, lanes, len(cands)


def reference_rows(nets, net_of, st, trig, scen, slot, k, n_ahead, spacing, radius):
    """lane_reference for the observers (scen[i], slot[i]) of a batch state (RolloutEngine.state(raw=True)); nets: LaneTables per
    network, net_of: per scenario its network or -1; trig [R, E, 2]: sin, cos of the headings."""
    out = []
    for r, e in zip(scen, slot):
        net = nets[net_of[r]] if net_of[r] >= 0 else None
        out.append(lane_reference(net, st["poses"][r, e, 0], st["poses"][r, e, 1], trig[r, e, 0], trig[r, e, 1], st["present"][r, e],
                                  k, n_ahead, spacing, radius))
    n, W = len(out), 6 + 2 * n_ahead
    return (np.array([o[0] for o in out]).reshape(n, k, W), np.array([o[1] for o in out], np.int32).reshape(n, k),
            np.array([o[2] for o in out], np.int32))


def trig_of(oracle, headings):
    """(sin, cos) of every heading by the oracle's sincos: [..., 2]."""
    h = np.asarray(headings, np.float64)
    return np.array([oracle.sincos(x) for x in h.ravel()]).reshape(h.shape + (2,))


def same(got, want):
    """feat bit for bit, lanes and count exactly."""
    return (got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
            and np.array_equal(got[2], want[2]))


def arrays_of(lanes, succ):
    """lane_arrays()-style arrays of lanes given as point lists and successor lists."""
    pts = [np.asarray(p, np.float64).reshape(-1, 2) for p in lanes]
    return dict(pt_off=np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64),
                pts=np.concatenate(pts) if pts else np.zeros((0, 2)),
                succ_off=np.concatenate([[0], np.cumsum([len(x) for x in succ])]).astype(np.int64),
                succ=np.array([q for x in succ for q in x], np.int32))


# the synthetic edge networks, shared by the hand-worked CPU test and the device test
EDGE_NETS = {
    "straight": arrays_of([[(0, 0), (10, 0)]], [[]]),
    # two lanes that share the end point (10, 0); a third far away
    "tie": arrays_of([[(0, 0), (10, 0)], [(10, 0), (10, 10)], [(40, 40), (50, 40)]], [[1], [], []]),
    # a successor chain that ends: 10 m then 5 m
    "chain": arrays_of([[(0, 0), (10, 0)], [(10, 0), (15, 0)]], [[1], []]),
    # two lanes that are each other's successor
    "loop": arrays_of([[(0, 0), (10, 0)], [(10, 0), (10, 10)]], [[1], [0]]),
    # lane 0's lowest-index successor is a one-point lane: lane 2 is taken; given out of order and twice
    "gap": arrays_of([[(0, 0), (10, 0)], [(10, 0)], [(10, 0), (10, 5)]], [[2, 1, 2], [], []]),
    # duplicated centre points: a zero-length first segment (lane 0), a zero-length last segment (lane 1)
    "dup": arrays_of([[(0, 0), (0, 0), (10, 0)], [(0, 20), (10, 20), (10, 20)]], [[], []]),
    "empty": arrays_of([], []),
}


def tables(arrs):
    return LaneTables(arrs["pt_off"], arrs["pts"], arrs["succ_off"], arrs["succ"])


# ---------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_the_lane_calls():
    """include/sgym.h declares the three calls with the issue's signatures, _lib.SYMBOLS names them, and the ABI version is
    still 7 (a purely additive change)."""
    import scenario_gym_amd._lib as L

    header = open(os.path.join(ROOT, "include", "sgym.h")).read()
    assert L.ABI_VERSION == 7 and re.search(r"#define SG_ABI_VERSION 7\b", header)
    assert re.search(r"\bint sg_set_lanes\(sg_handle \*h, const sg_lanes \*lanes\);", header) and "sg_set_lanes" in L.SYMBOLS
    st = re.search(r"typedef struct sg_lanes \{(.*?)\} sg_lanes;", header, re.S).group(1)
    assert re.findall(r"\b(\w+);", st) == ["n_networks", "lane_off", "pt_off", "pts", "succ_off", "succ"]
    assert [n for n, _ in L.SgLanes._fields_] == ["n_networks", "lane_off", "pt_off", "pts", "succ_off", "succ"]
    for name in ("sg_lane_observation", "sg_lane_observation_observers"):
        assert name in L.SYMBOLS
        assert re.search(r"\bint " + name + r"\(sg_handle \*h, int32_t k, int32_t n_ahead, double spacing, double radius,\s*double \*feat, "
                         r"int32_t \*lanes, int32_t \*count,\s*int32_t outputs_device\);", header), name


def test_yardstick_on_hand_made_scenes():
    """The numpy restatement on scenes whose answers are worked out by hand (heading 0: sin 0, cos 1)."""
    ref = lambda net, px, py, k=1, n_ahead=0, spacing=2.0, radius=INF, s=0.0, c=1.0, present=True: \
        lane_reference(net, px, py, s, c, present, k, n_ahead, spacing, radius)  # noqa: E731
    # a straight lane along +x, the observer 2 m to its left at arclength 3
    net = tables(EDGE_NETS["straight"])
    f, l, n = ref(net, 3, 2, n_ahead=3)
    assert n == 1 and l.tolist() == [0] and f[0].tolist() == [2, 1, 0, 3, 7, 2, 2, -2, 4, -2, 6, -2]
    # heading pi / 2 (sin 1, cos 0): the lane runs to the observer's right, the points ahead turn with the frame
    f, l, n = ref(net, 3, 2, n_ahead=1, s=1.0, c=0.0)
    assert f[0].tolist() == [2, 0, 1, 3, 7, 2, -2, -2]
    # before the start and past the end: the clamps; the distance [5] is not |lateral| [0] there
    f, l, n = ref(net, -3, 4, n_ahead=1)
    assert f[0].tolist() == [4, 1, 0, 0, 10, 5, 5, -4]
    f, l, n = ref(net, 13, 4, n_ahead=1)
    assert f[0].tolist() == [4, 1, 0, 10, 0, 5, -3, -4]  # (the point ahead holds at the lane's last point)
    # the radius is inclusive: the lane AT 2 is kept, one ulp less drops it
    assert ref(net, 3, 2, radius=2.0)[2] == 1 and ref(net, 3, 2, radius=2.0)[1].tolist() == [0]
    f, l, n = ref(net, 3, 2, k=2, radius=np.nextafter(2.0, 0.0))
    assert n == 0 and l.tolist() == [-1, -1] and not f.any() and not np.signbit(f).any()
    # an absent observer, a scenario without a network
    f, l, n = ref(net, 3, 2, k=2, n_ahead=2, present=False)
    assert n == -1 and l.tolist() == [-1, -1] and f.shape == (2, 10) and not f.any() and not np.signbit(f).any()
    f, l, n = ref(None, 3, 2, k=2)
    assert n == 0 and l.tolist() == [-1, -1] and not f.any()
    # two lanes share (10, 0) and the observer is nearest that vertex: an exact tie, the lower index first; count tells of the third
    net = tables(EDGE_NETS["tie"])
    f, l, n = ref(net, 12, -2, k=2)
    assert n == 3 and l.tolist() == [0, 1] and f[0, 5] == f[1, 5] == math.sqrt(8.0) and f[0, 3] == 10 and f[1, 3] == 0
    assert ref(net, 12, -2, k=3, radius=3.0)[1].tolist() == [0, 1, -1] and ref(net, 12, -2, k=3, radius=3.0)[2] == 2
    # a successor chain shorter than the look-ahead: 8 on lane 0, 13 = 3 into lane 1, then the chain's last point
    net = tables(EDGE_NETS["chain"])
    f, l, n = ref(net, 3, 0, n_ahead=4, spacing=5.0)
    assert l.tolist() == [0] and f[0, 6:].tolist() == [5, 0, 10, 0, 12, 0, 12, 0]
    # a two-lane loop, from arclength 0 in steps of 15: 5 into lane 1; exactly the end of lane 0 after two hops; 5 into lane 0
    # after four; and 60 = 20 left after four hops: the cap stops the walk at lane 0's last point
    net = tables(EDGE_NETS["loop"])
    f, l, n = ref(net, 0, 0, n_ahead=4, spacing=15.0)
    assert l.tolist() == [0] and f[0, 6:].tolist() == [10, 5, 10, 0, 5, 0, 10, 0]
    # lane 0's lowest-index successor has no segments: the next one is taken; the one-point lane is never chosen; fewer lanes than k
    net = tables(EDGE_NETS["gap"])
    assert net.succ[0] == [1, 2] and not net.has_segments(1)
    f, l, n = ref(net, 8, 0, k=4, n_ahead=1, spacing=5.0)
    assert n == 2 and l.tolist() == [0, 2, -1, -1] and f[0, 6:].tolist() == [2, 3] and not f[2:].any()
    # a duplicated centre point.  Lane 0 starts with a zero-length segment, which is the best one (the tie goes to the lower
    # segment index): the direction features are 0; spacing 0 puts the point ahead on the LAST segment with cum <= 0
    net = tables(EDGE_NETS["dup"])
    f, l, n = ref(net, -3, 4, n_ahead=1, spacing=0.0)
    assert l.tolist() == [0] and f[0].tolist() == [0, 0, 0, 0, 10, 5, 3, -4] and not np.signbit(f[0, :3]).any()
    # lane 1 ends with one: the target 10 = cum of the zero-length segment gives u = 0, its point a
    f, l, n = ref(net, 4, 20, n_ahead=2, spacing=6.0)
    assert l.tolist() == [1] and f[0].tolist() == [0, 1, 0, 4, 6, 0, 6, 0, 6, 0]
    # a network without lanes
    assert ref(tables(EDGE_NETS["empty"]), 1, 1, k=2)[2] == 0


@pytest.fixture(scope="module")
def networks(reference_inputs):
    """The six fixture networks by name (loaded once)."""
    from scenario_gym_amd.road_network import RoadNetwork

    return {n: RoadNetwork.create_from_json(os.path.join(reference_inputs, "Road_Networks", n + ".json")) for n in FIXTURE_COUNTS}


def test_lane_arrays_of_the_fixture_networks(networks):
    """RoadNetwork.lane_arrays() on the six networks: the lane and point counts, monotone offsets, lane q = lanes[q], successors
    ascending, in range, each once, and those of the lane graph."""
    pts_per_lane = []
    for name, (n_lanes, n_pts) in FIXTURE_COUNTS.items():
        rn = networks[name]
        a = rn.lane_arrays()
        assert a is rn.lane_arrays()
        assert len(rn.lanes) == n_lanes == len(a["pt_off"]) - 1 == len(a["succ_off"]) - 1 and a["pts"].shape == (n_pts, 2)
        assert a["pt_off"][0] == 0 and a["pt_off"][-1] == n_pts and (np.diff(a["pt_off"]) >= 0).all()
        assert a["succ_off"][0] == 0 and a["succ_off"][-1] == len(a["succ"]) and (np.diff(a["succ_off"]) >= 0).all()
        assert a["pts"].dtype == np.float64 and a["succ"].dtype == np.int32 and a["pt_off"].dtype == a["succ_off"].dtype == np.int64
        index = {l.id: q for q, l in enumerate(rn.lanes)}
        for q, l in enumerate(rn.lanes):
            got = a["pts"][a["pt_off"][q]:a["pt_off"][q + 1]]
            assert np.array_equal(got, l.center) and len(got) >= 2
            s = a["succ"][a["succ_off"][q]:a["succ_off"][q + 1]].tolist()
            assert s == sorted(set(s)) and all(0 <= z < n_lanes for z in s)
            assert s == sorted({index[i] for i in l.successors if i in index})
        seg = np.diff(a["pts"], axis=0)
        inner = np.ones(len(seg), bool)
        inner[a["pt_off"][1:-1] - 1] = False  # (the differences across two lanes)
        assert (np.hypot(seg[:, 0], seg[:, 1])[inner] > 0).all()  # no zero-length segment
        pts_per_lane += np.diff(a["pt_off"]).tolist()
    assert (min(pts_per_lane), max(pts_per_lane)) == (8, 1055)


def test_lane_arrays_drop_what_the_device_cannot_use():
    """A lane without a centre or with a single point has no points; unknown successor ids and duplicates are dropped."""
    from scenario_gym_amd.road_network import Lane, Road, RoadNetwork

    def lane(i, center, successors):
        l = Lane(i, np.zeros((3, 2)), center=center)
        l.successors, l.predecessors, l.type = successors, [], "driving"
        return l

    road = Road("r", np.zeros((3, 2)))
    road.lanes = [lane("a", [(0, 0), (1, 0), (2, 0)], ["c", "nowhere", "b", "c"]), lane("b", None, []), lane("c", [(5, 5)], ["a"])]
    rn = RoadNetwork(roads=[road], lanes=[lane("d", [(0, 1), (0, 2)], ["a", "d"])])
    a = rn.lane_arrays()
    assert [l.id for l in rn.lanes] == ["a", "b", "c", "d"]
    assert a["pt_off"].tolist() == [0, 3, 3, 3, 5] and a["pts"].tolist() == [[0, 0], [1, 0], [2, 0], [0, 1], [0, 2]]
    assert a["succ_off"].tolist() == [0, 2, 2, 3, 5] and a["succ"].tolist() == [1, 2, 0, 0, 3]


def test_shared_lane_arrays(networks):
    """One network object shared between scenarios goes down once, with the net_of of shared_polygon_arrays."""
    from scenario_gym_amd.road_network import shared_lane_arrays, shared_polygon_arrays

    class Sc:
        def __init__(self, rn):
            self.road_network = rn

    a, b = networks[SMALLEST], networks[RURAL]
    scs = [Sc(a), Sc(None), Sc(b), Sc(a), Sc(b), Sc(None)]
    nets, net_of = shared_lane_arrays(scs)
    assert net_of == [0, -1, 1, 0, 1, -1] == shared_polygon_arrays(scs)[1]
    assert len(nets) == 2 and nets[0] is a.lane_arrays() and nets[1] is b.lane_arrays()
    assert shared_lane_arrays([]) == ([], [])


# ---------------------------------------------------------------------------------------------------- GPU: the C ABI
def _ff(shape, dtype):
    """A host array whose every byte is 0xFF."""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xFF, np.uint8).view(dtype).reshape(shape)


def _raw(eng, n, k, n_ahead, spacing, radius, observers, want_lanes=True, want_count=True):
    """One of the two calls through ctypes into 0xFF-filled host buffers of n observers: (rc, feat, lanes, count)."""
    feat, lanes, count = _ff((n, k, 6 + 2 * n_ahead), np.float64), _ff((n, k), np.int32), _ff((n,), np.int32)
    call = eng.lib.sg_lane_observation_observers if observers else eng.lib.sg_lane_observation
    rc = call(eng.h, k, n_ahead, spacing, radius, feat.ctypes.data, lanes.ctypes.data if want_lanes else None,
              count.ctypes.data if want_count else None, 0)
    return rc, feat, lanes, count


def _untouched(*arrays):
    return all((a.view(np.uint8) == 0xFF).all() for a in arrays)


def _no_polygons():
    return dict(ring_off=np.zeros(1, np.int64), vert_off=np.zeros(1, np.int64), verts=np.zeros((0, 2)), layers=np.zeros(0, np.uint32))


@pytest.fixture(scope="module")
def reference_batch(networks):
    """The four reference rollouts of roads.npz -- on the 6-lane intersection (132 lanes, 11,040 points: more than 64 segments
    per wavefront lane, more than 64 road lanes), the roundabout, the rural network (a lane of 1,055 points) and Greenwich 002
    -- as one batch: (packed, road networks per scenario, LaneTables per scenario)."""
    from scenario_gym_amd.packing import pack_arrays

    g = load_golden("roads")
    names = [str(x) for x in g["scenarios"]]
    rns = [networks[str(g[f"{n}/network"])] for n in names]
    assert {SIX_LANE, RURAL} <= {str(g[f"{n}/network"]) for n in names}
    packed = pack_arrays([scenario_arrays(g, f"{n}/scenario") for n in names])
    return packed, rns, [tables(rn.lane_arrays()) for rn in rns]


def _reference_engine(sga, reference_batch, steps=5):
    packed, rns, tabs = reference_batch
    eng = sga.RolloutEngine(packed.n_scenarios, packed.n_entities, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks([rn.polygon_arrays() for rn in rns], np.arange(len(rns)))
    eng.set_lanes([rn.lane_arrays() for rn in rns])
    eng.step(steps)
    return eng, eng.state(raw=True), tabs, np.arange(len(rns)), packed.ego.copy()


@gpu
def test_egos_of_the_reference_scenarios(sga, oracle, reference_batch):
    """The ego call on the reference scenarios, stepped five ticks: k = 1, 3, 8, n_ahead = 0, 4, 16, spacing 2 and 40 (several
    successors per point), radius inf and 5."""
    eng, st, tabs, net_of, ego = _reference_engine(sga, reference_batch)
    trig = trig_of(oracle, st["poses"][..., 3])
    R = len(ego)
    assert st["present"][np.arange(R), ego].all()
    full = cut = hopped = 0
    for k in (1, 3, 8):
        for n_ahead in (0, 4, 16):
            for spacing in (2.0, 40.0):
                for radius in (INF, 5.0):
                    rc, *got = _raw(eng, R, k, n_ahead, spacing, radius, observers=False)
                    want = reference_rows(tabs, net_of, st, trig, np.arange(R), ego, k, n_ahead, spacing, radius)
                    assert rc == 0 and same(got, want), (k, n_ahead, spacing, radius)
                    full += int((want[2] > k).sum())
                    cut += int(((want[1] == -1).any(axis=1) & (want[2] >= 0)).sum())
                    if n_ahead and spacing == 40.0:  # a point further ahead than what is left of the lane: the walk left it
                        hopped += int((want[0][:, 0, 4] < 40.0 * n_ahead).sum())
    assert full > 0 and cut > 0 and hopped > 0
    assert [t.n_lanes for t in tabs].count(132) == 1 and max(t.n_lanes for t in tabs) == 132
    eng.close()


@gpu
def test_every_entity_of_the_reference_scenarios_observes(sga, oracle, reference_batch):
    """Every entity slot that holds an entity as an observer, some twice and out of order; the observer (r, ego of r) reproduces
    the ego call's bytes; entities that are not in the scene (not spawned yet after five ticks, or vanished after 150) get
    count -1, lanes -1 and zeros."""
    packed, _, _ = reference_batch
    eng, st, tabs, net_of, ego = _reference_engine(sga, reference_batch)
    R, E = packed.n_scenarios, packed.n_entities
    held = np.argwhere(packed.kind.reshape(R, E) != 0)
    scen = np.concatenate([np.arange(R), held[:, 0], held[::-3, 0]]).astype(np.int32)
    slot = np.concatenate([ego, held[:, 1], held[::-3, 1]]).astype(np.int32)
    eng.set_observers(scen, slot)
    absent = 0
    for steps in (0, 145):
        if steps:
            eng.step(steps)
            st = eng.state(raw=True)
        trig = trig_of(oracle, st["poses"][..., 3])
        for k, n_ahead, spacing, radius in ((8, 4, 2.0, INF), (3, 16, 40.0, 5.0), (1, 0, 2.0, 30.0)):
            rc, *got = _raw(eng, len(scen), k, n_ahead, spacing, radius, observers=True)
            want = reference_rows(tabs, net_of, st, trig, scen, slot, k, n_ahead, spacing, radius)
            assert rc == 0 and same(got, want), (steps, k, n_ahead, spacing, radius)
            rc, *egos = _raw(eng, R, k, n_ahead, spacing, radius, observers=False)
            assert rc == 0 and all(a[:R].tobytes() == b.tobytes() for a, b in zip(got, egos))
            gone = ~st["present"][scen, slot]
            assert (got[2][gone] == -1).all() and (got[1][gone] == -1).all() and not got[0][gone].any()
            absent += int(gone.sum())
    assert absent > 0
    eng.close()


def _edge_batch(sga):
    """Six scenarios of four standing entities each on the synthetic edge networks -- the tie, the loop, the duplicated points,
    the successor without segments (two lanes with segments: fewer than k), a network with no lanes, no network -- with the ego
    in slot 1 and the last entity not spawned yet.  Returns (engine, state, LaneTables per network, net_of)."""
    from scenario_gym_amd.packing import pack_arrays

    names = ["tie", "loop", "dup", "gap", "empty"]
    net_of = np.array([0, 1, 2, 3, 4, -1], np.int32)
    spots = [[(12, -2, 0.3), (10, 0, 2.0), (3, 1, -1.0), (9, 9, 0.0)],       # at the shared vertex's corner, ON it
             [(0, 0, 0.0), (2, -1, 0.5), (10, 4, 1.5), (5, 5, 0.0)],
             [(-3, 4, 0.0), (4, 20, 0.1), (0, 0, 3.0), (10, 20.5, 0.0)],     # the zero-length segments are the nearest
             [(8, 0, 0.0), (10, 0.5, 1.0), (11, 3, -2.0), (0, 0, 0.0)],
             [(1, 1, 0.0), (2, 2, 0.0), (3, 3, 0.0), (4, 4, 0.0)],
             [(1, 1, 0.0), (2, 2, 0.0), (3, 3, 0.0), (4, 4, 0.0)]]
    scs = []
    for sp in spots:
        knots, off = [], [0]
        for i, (x, y, h) in enumerate(sp):
            for t in ((5.0 if i == 3 else 0.0), 10.0):
                knots.append([t, x, y, 0.0, h, 0.0, 0.0])
            off.append(len(knots))
        scs.append(dict(knot_off=np.array(off, np.int64), knots=np.array(knots, np.float64), bbox=np.tile([2.0, 4.5, 0.0, 0.0], (4, 1)),
                        etype=np.zeros(4, np.int32), ego=1, t0=0.0, length=10.0))
    eng = sga.RolloutEngine(6, 4, timestep=0.1)
    eng.upload(pack_arrays(scs))
    eng.set_road_networks([_no_polygons() for _ in names], net_of)
    eng.set_lanes([EDGE_NETS[n] for n in names])
    eng.step(2)
    st = eng.state(raw=True)
    assert st["present"][:, :3].all() and not st["present"][:, 3].any()
    return eng, st, [tables(EDGE_NETS[n]) for n in names], net_of


@gpu
def test_synthetic_edge_networks(sga, oracle):
    """The edge networks of the hand-worked test through sg_set_lanes: the exact tie at a shared vertex, the hop cap in a successor
    loop, zero-length segments, fewer lanes than k, the successor without segments, a network with zero lanes and a scenario
    without a network beside the others; the egos and every slot as an observer."""
    eng, st, tabs, net_of = _edge_batch(sga)
    trig = trig_of(oracle, st["poses"][..., 3])
    scen, slot = np.repeat(np.arange(6), 4).astype(np.int32), np.tile(np.arange(4), 6).astype(np.int32)
    eng.set_observers(scen, slot)
    for k, n_ahead, spacing, radius in ((3, 4, 15.0, INF), (8, 16, 6.0, INF), (2, 2, 0.0, 3.0), (1, 0, 2.0, 0.0), (4, 3, 1e300, INF)):
        rc, *got = _raw(eng, len(scen), k, n_ahead, spacing, radius, observers=True)
        want = reference_rows(tabs, net_of, st, trig, scen, slot, k, n_ahead, spacing, radius)
        assert rc == 0 and same(got, want), (k, n_ahead, spacing, radius)
        rc, *egos = _raw(eng, 6, k, n_ahead, spacing, radius, observers=False)
        assert rc == 0 and same(egos, reference_rows(tabs, net_of, st, trig, np.arange(6), np.ones(6, np.int32), k, n_ahead, spacing, radius))
        if k == 3 and radius == INF:
            lanes, count = want[1].reshape(6, 4, k), want[2].reshape(6, 4)
            assert lanes[0, 0].tolist() == [0, 1, 2] and lanes[0, 1].tolist() == [0, 1, 2]  # the tie: the lower index first
            assert want[0].reshape(6, 4, k, -1)[0, 0, 0, 5] == want[0].reshape(6, 4, k, -1)[0, 0, 1, 5]
            assert count[3, :3].tolist() == [2, 2, 2] and (lanes[3, :3, 2] == -1).all() and not (lanes[3, :3, :2] == 1).any()
            assert count[4].tolist() == [0, 0, 0, -1] and count[5].tolist() == [0, 0, 0, -1] and count[2, :3].tolist() == [2, 2, 2]
            assert want[0].reshape(6, 4, k, -1)[2, 0, 0, :3].tolist() == [0, 0, 0]  # the zero-length best segment
    eng.close()


@gpu
@pytest.mark.parametrize("E", [70, 530])
def test_wide_scenarios(sga, oracle, networks, E):
    """Scenarios of more than 64 and of more than 512 entity slots: only the addressing of the observer's row differs.  Two
    scenarios on the smallest fixture network; the egos, and observers all over the slots."""
    from scenario_gym_amd import synthetic

    rn = networks[SMALLEST]
    v = rn.polygon_arrays()["verts"]
    packed = synthetic.make_batch(2, E, n_steps=30, timestep=0.1, n_knots=16, extent=float((v.max(0) - v.min(0)).min()) / 2, vanish_frac=0.3, seed=E)
    packed.knots[:, 1:3] += (v.max(0) + v.min(0)) / 2
    eng = sga.RolloutEngine(2, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks([rn.polygon_arrays()], [0, 0])
    eng.set_lanes([rn.lane_arrays()])
    eng.step(4)
    st = eng.state(raw=True)
    trig = trig_of(oracle, st["poses"][..., 3])
    tabs = [tables(rn.lane_arrays())]
    pick = np.unique(np.concatenate([np.arange(0, E, 7), [63, 64, 65, E - 1]]))
    scen = np.concatenate([np.zeros(len(pick)), np.ones(len(pick))]).astype(np.int32)
    slot = np.concatenate([pick, pick]).astype(np.int32)
    assert not st["present"][scen, slot].all() and st["present"][scen, slot].sum() > 10
    eng.set_observers(scen, slot)
    for k, n_ahead, spacing, radius in ((8, 4, 2.0, INF), (2, 16, 25.0, 10.0)):
        rc, *got = _raw(eng, len(scen), k, n_ahead, spacing, radius, observers=True)
        want = reference_rows(tabs, [0, 0], st, trig, scen, slot, k, n_ahead, spacing, radius)
        assert rc == 0 and same(got, want) and (want[2] > 0).any(), (k, n_ahead, spacing, radius)
        rc, *got = _raw(eng, 2, k, n_ahead, spacing, radius, observers=False)
        assert rc == 0 and same(got, reference_rows(tabs, [0, 0], st, trig, [0, 1], packed.ego, k, n_ahead, spacing, radius))
    eng.close()


@gpu
def test_output_paths_and_buffers(sga, oracle, reference_batch):
    """Device outputs equal host outputs and are queued behind a step; every byte of 0xFF-filled buffers is rewritten; NULL lanes /
    count leave the rest correct; with no observers the buffers stay untouched."""
    import torch

    packed, _, _ = reference_batch
    eng, st, tabs, net_of, ego = _reference_engine(sga, reference_batch)
    R, E, k, n_ahead, spacing, radius = packed.n_scenarios, packed.n_entities, 3, 4, 10.0, 8.0
    W = 6 + 2 * n_ahead
    rc, *none = _raw(eng, 4, k, n_ahead, spacing, radius, observers=True)
    assert rc == 0 and _untouched(*none)  # no observers set
    assert eng.lib.sg_lane_observation_observers(eng.h, k, n_ahead, spacing, radius, None, None, None, 0) == 0
    held = np.argwhere(packed.kind.reshape(R, E) != 0)
    scen, slot = held[:, 0].astype(np.int32), held[:, 1].astype(np.int32)
    eng.set_observers(scen, slot)
    n = len(scen)
    trig = trig_of(oracle, st["poses"][..., 3])
    want = reference_rows(tabs, net_of, st, trig, scen, slot, k, n_ahead, spacing, radius)
    rc, *host = _raw(eng, n, k, n_ahead, spacing, radius, observers=True)
    assert rc == 0 and same(host, want) and (want[1] == -1).any() and (want[2] == -1).any()  # (zero rows and -1 were written over 0xFF)
    rc, *egos = _raw(eng, R, k, n_ahead, spacing, radius, observers=False)
    assert rc == 0 and same(egos, reference_rows(tabs, net_of, st, trig, np.arange(R), ego, k, n_ahead, spacing, radius))
    # NULL lanes / count: the features alone, the other buffers untouched
    rc, f, l, c = _raw(eng, n, k, n_ahead, spacing, radius, observers=True, want_lanes=False, want_count=False)
    assert rc == 0 and f.tobytes() == host[0].tobytes() and _untouched(l, c)
    rc, f, l, c = _raw(eng, R, k, n_ahead, spacing, radius, observers=False, want_lanes=False)
    assert rc == 0 and f.tobytes() == egos[0].tobytes() and _untouched(l) and np.array_equal(c, egos[2])
    rc, f, l, c = _raw(eng, R, k, n_ahead, spacing, radius, observers=False, want_count=False)
    assert rc == 0 and f.tobytes() == egos[0].tobytes() and np.array_equal(l, egos[1]) and _untouched(c)
    # device outputs through the engine, and raw into 0xFF-filled tensors queued right behind a step
    for dev, ref in ((eng.lane_observation_observers(k, n_ahead, spacing, radius, torch_out=True), host),
                     (eng.lane_observation(k, n_ahead, spacing, radius, torch_out=True), egos)):
        assert all(t.is_cuda for t in dev) and (dev[0].dtype, dev[1].dtype, dev[2].dtype) == (torch.float64, torch.int32, torch.int32)
        assert same([t.cpu().numpy() for t in dev], ref)
    assert same(eng.lane_observation_observers(k, n_ahead, spacing, radius), host) and same(eng.lane_observation(k, n_ahead, spacing, radius), egos)
    d_feat = torch.full((n * k * W * 8,), 0xFF, dtype=torch.uint8, device="cuda:0")
    d_lanes = torch.full((n * k * 4,), 0xFF, dtype=torch.uint8, device="cuda:0")
    d_count = torch.full((n * 4,), 0xFF, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert eng.lib.sg_step(eng.h, 3, None, 0) == 0
    assert eng.lib.sg_lane_observation_observers(eng.h, k, n_ahead, spacing, radius, d_feat.data_ptr(), d_lanes.data_ptr(), d_count.data_ptr(), 1) == 0
    assert eng.lib.sg_synchronize(eng.h) == 0
    st2 = eng.state(raw=True)
    want2 = reference_rows(tabs, net_of, st2, trig_of(oracle, st2["poses"][..., 3]), scen, slot, k, n_ahead, spacing, radius)
    got2 = (d_feat.cpu().numpy().view(np.float64).reshape(n, k, W), d_lanes.cpu().numpy().view(np.int32).reshape(n, k),
            d_count.cpu().numpy().view(np.int32))
    assert same(got2, want2) and not same(want2, want)
    eng.set_observers([], [])
    rc, *none = _raw(eng, n, k, n_ahead, spacing, radius, observers=True)
    assert rc == 0 and _untouched(*none)
    assert same(eng.lane_observation_observers(k, n_ahead, spacing, radius), (np.zeros((0, k, W)), np.zeros((0, k), np.int32), np.zeros(0, np.int32)))
    eng.close()


def _set_lanes_raw(eng, n_networks, lane_off, pt_off, pts, succ_off, succ):
    import ctypes as C

    import scenario_gym_amd._lib as L

    keep = [None if a is None else np.ascontiguousarray(a, dt) for a, dt in
            ((lane_off, np.int64), (pt_off, np.int64), (pts, np.float64), (succ_off, np.int64), (succ, np.int32))]
    st = L.SgLanes(n_networks, *[None if a is None else a.ctypes.data for a in keep])
    return eng.lib.sg_set_lanes(eng.h, C.byref(st))


@gpu
def test_lifecycle_and_refusals(sga, oracle, reference_batch):
    """Before sg_set_lanes the call gives count 0; sg_upload and a second sg_set_road_networks forget the lanes; every refusal of
    sg_set_lanes and of the two observation calls comes with a message that names the call, and the handle answers afterwards."""
    packed, rns, tabs = reference_batch
    R = packed.n_scenarios
    net_of = np.arange(R)
    poly, lanes = [rn.polygon_arrays() for rn in rns], [rn.lane_arrays() for rn in rns]
    good = (1, [0, 2], [0, 2, 4], [[0, 0], [1, 0], [1, 0], [1, 1]], [0, 1, 1], [1])

    def refused(eng, rc, want, name):
        return rc == want and eng.lib.sg_last_error(eng.h).decode().startswith(name + ":")

    def empty(got):
        return (got[2] == 0).all() and (got[1] == -1).all() and not got[0].any() and not np.signbit(got[0]).any()

    eng = sga.RolloutEngine(R, packed.n_entities, timestep=0.1)
    for observers, name in ((False, "sg_lane_observation"), (True, "sg_lane_observation_observers")):
        assert refused(eng, _raw(eng, R, 2, 2, 2.0, INF, observers)[0], SG_ERR_STATE, name)
    assert refused(eng, _set_lanes_raw(eng, *good), SG_ERR_STATE, "sg_set_lanes")  # before sg_upload
    eng.upload(packed)
    eng.reset()
    assert refused(eng, _set_lanes_raw(eng, *good), SG_ERR_STATE, "sg_set_lanes")  # before sg_set_road_networks
    rc, *got = _raw(eng, R, 2, 2, 2.0, INF, observers=False)
    assert rc == 0 and empty(got)  # no networks, no lanes
    eng.set_road_networks(poly, net_of)
    rc, *got = _raw(eng, R, 2, 2, 2.0, INF, observers=False)
    assert rc == 0 and empty(got)  # networks, but no lanes yet
    eng.set_lanes(lanes)
    st = eng.state(raw=True)
    trig = trig_of(oracle, st["poses"][..., 3])
    want = reference_rows(tabs, net_of, st, trig, np.arange(R), packed.ego, 2, 2, 2.0, INF)
    rc, *got = _raw(eng, R, 2, 2, 2.0, INF, observers=False)
    assert rc == 0 and same(got, want) and (want[2] > 0).all()
    # refusals of sg_set_lanes leave the lanes that are set
    one = eng.lib.sg_set_lanes
    assert refused(eng, one(eng.h, None), SG_ERR_INVALID, "sg_set_lanes")
    four = lambda **kw: _set_lanes_raw(eng, **{**dict(n_networks=R, lane_off=[0, 1, 2, 3, 4], pt_off=[0, 2, 4, 6, 8], pts=np.arange(16.0),  # noqa: E731
                                                    succ_off=[0, 1, 1, 1, 1], succ=[0]), **kw})
    assert four() == 0
    rc, *got = _raw(eng, R, 2, 0, 2.0, INF, observers=False)
    assert rc == 0 and (got[2] == 1).all() and (got[1] == [0, -1]).all()
    eng.set_lanes(lanes)
    for kw in (dict(n_networks=R - 1), dict(n_networks=R + 1), dict(lane_off=[0, 2, 1, 3, 4]), dict(lane_off=[1, 1, 2, 3, 4]),
               dict(pt_off=[0, 2, 1, 6, 8]), dict(succ_off=[0, 1, 0, 1, 1]), dict(succ=[1]), dict(succ=[-1]), dict(lane_off=None),
               dict(pt_off=None), dict(succ_off=None), dict(pts=None), dict(succ=None)):
        assert refused(eng, four(**kw), SG_ERR_INVALID, "sg_set_lanes"), kw
        rc, *got = _raw(eng, R, 2, 2, 2.0, INF, observers=False)
        assert rc == 0 and same(got, want), kw
    # refusals of the observation calls
    eng.set_observers([0, 1], [0, 0])
    for observers, name in ((False, "sg_lane_observation"), (True, "sg_lane_observation_observers")):
        call = getattr(eng.lib, name)
        for k, n_ahead, spacing, radius in ((0, 2, 2.0, INF), (9, 2, 2.0, INF), (-1, 2, 2.0, INF), (2, -1, 2.0, INF), (2, 17, 2.0, INF),
                                            (2, 2, -1.0, INF), (2, 2, float("nan"), INF), (2, 2, INF, INF), (2, 2, 2.0, -1.0),
                                            (2, 2, 2.0, float("nan"))):
            feat = _ff((R, 9, 40), np.float64)
            assert refused(eng, call(eng.h, k, n_ahead, spacing, radius, feat.ctypes.data, None, None, 0), SG_ERR_INVALID, name), (k, n_ahead, spacing, radius)
            assert _untouched(feat)
        assert refused(eng, call(eng.h, 2, 2, 2.0, INF, None, None, None, 0), SG_ERR_INVALID, name)
    rc, *got = _raw(eng, R, 2, 2, 2.0, INF, observers=False)
    assert rc == 0 and same(got, want)
    # a second sg_set_road_networks forgets the lanes, and so does sg_upload
    eng.set_road_networks(poly, net_of)
    rc, *got = _raw(eng, R, 2, 2, 2.0, INF, observers=False)
    assert rc == 0 and empty(got)
    eng.set_lanes(lanes)
    assert same(_raw(eng, R, 2, 2, 2.0, INF, observers=False)[1:], want)
    eng.upload(packed)
    eng.reset()
    rc, *got = _raw(eng, R, 2, 2, 2.0, INF, observers=False)
    assert rc == 0 and empty(got)
    eng.set_road_networks(poly, net_of)
    eng.set_lanes(lanes)
    assert same(_raw(eng, R, 2, 2, 2.0, INF, observers=False)[1:], want)
    eng.close()


# ---------------------------------------------------------------------------------------------------- GPU: the Python layers
def _reference_scenarios(networks):
    g = load_golden("roads")
    scs = []
    for n in (str(x) for x in g["scenarios"]):
        sc = scenario_from_arrays(scenario_arrays(g, f"{n}/scenario"), g[f"{n}/scenario/refs"])
        sc.road_network = networks[str(g[f"{n}/network"])]
        scs.append(sc)
    return scs


@gpu
def test_state_and_sensors(sga, networks):
    """State.lane_observation, LaneSensor alone on the ego's agent and inside a CombinedSensor on another entity's, and a sensor
    stepped by the caller: what each saw equals the engine call on that state, and the lanes are the objects of
    RoadNetwork.lanes.  A scenario without a road network sees no lanes."""
    sc = _reference_scenarios(networks)[0]
    rn = sc.road_network
    t0 = sc.ego.trajectory.min_t  # (the scenario starts when its ego does); another entity that is in the scene for the first second
    other_ref = next(e.ref for e in sc.entities if e is not sc.ego and e.trajectory.min_t <= t0 and e.trajectory.max_t >= t0 + 1.0)
    index = {e.ref: j for j, e in enumerate(sc.entities)}
    log = []
    gym = sga.ScenarioGym(timestep=0.1)

    class Watcher(sga.Agent):
        def __init__(self, entity, sensor):
            super().__init__(entity, sga.ReplayTrajectoryController(entity), sensor)

        def _step(self, obs):
            if self.entity.ref == "ego":
                f, l, c = gym._b.engine.lane_observation(4, 3, 5.0, 30.0)
                o = 0
            else:
                f, l, c = gym._b.engine.lane_observation_observers(2, 1, 2.0, INF)
                o = gym._b._observer_of[(0, index[self.entity.ref])]
            log.append((self.entity, obs, f[o], l[o], c[o]))
            return sga.TeleportAction(pose=self.entity.trajectory.position_at_t(obs.next_t))

    def create_agent(s, e):
        if e.ref == "ego":
            return Watcher(e, sga.LaneSensor(e, k=4, n_ahead=3, spacing=5.0, radius=30.0))
        if e.ref == other_ref:
            return Watcher(e, sga.CombinedSensor(e, sga.LaneSensor(e, k=2, n_ahead=1), sga.NearestEntitiesSensor(e, k=2)))

    gym.set_scenario(sc, create_agent=create_agent)
    ents = gym.state.scenario.entities
    loose = sga.LaneSensor(ents[index[other_ref]], k=3, n_ahead=2, spacing=1.0, radius=50.0)  # stepped by the caller
    assert loose.output_shape == (3, 10)
    for _ in range(5):
        gym.step()
        obs = loose.step(gym.state)
        f, l, c = gym._b.engine.lane_observation_observers(3, 2, 1.0, 50.0)
        o = gym._b._observer_of[(0, index[other_ref])]
        assert isinstance(obs, sga.LaneObservation) and obs.lane_features.tobytes() == f[o].tobytes()
        assert len(obs.lanes) == min(c[o], 3) > 0 and all(a is rn.lanes[j] for a, j in zip(obs.lanes, l[o]))
        lanes, feat = gym.state.lane_observation(4, 3, 5.0, 30.0)
        fe, le, ce = gym._b.engine.lane_observation(4, 3, 5.0, 30.0)
        assert feat.tobytes() == fe[0].tobytes() and all(a is rn.lanes[j] for a, j in zip(lanes, le[0])) and len(lanes) == min(ce[0], 4)
        assert gym.state.lane_observation(4, 3, 5.0, 30.0, entity=gym.state.scenario.ego)[0] == lanes
    gym.close()
    seen = 0
    for entity, obs, f, l, c in log:
        assert obs.lane_features.shape == ((4, 12) if entity.ref == "ego" else (2, 8)) and obs.lane_features.tobytes() == f.tobytes()
        assert len(obs.lanes) == min(c, len(l)) and all(a is rn.lanes[j] for a, j in zip(obs.lanes, l)) and obs.entity is entity
        if entity.ref != "ego":
            assert obs.features.shape == (2, 8) and isinstance(obs.neighbours, list)  # (the nearest-entity sensor beside it)
        seen += len(obs.lanes)
    assert len(log) >= 8 and seen > 10
    # no road network: no lanes, zeros
    bare = _reference_scenarios(networks)[1]
    bare.road_network = None
    gym = sga.ScenarioGym(timestep=0.1)
    gym.set_scenario(bare)
    gym.step()
    lanes, feat = gym.state.lane_observation(2, 1)
    assert lanes == [] and feat.shape == (2, 8) and not feat.any()
    gym.close()


@gpu
def test_vector_env(sga, oracle, networks):
    """VectorScenarioEnv.lane_observation / observe_entities_lanes, numpy and torch forms: the yardstick on the state the
    environment is in; the lanes go down on first use, and construction, reset and step behave as before."""
    scs = _reference_scenarios(networks)
    tabs = [tables(sc.road_network.lane_arrays()) for sc in scs]
    net_of = np.arange(len(scs))
    ego = np.array([sc.entities.index(sc.ego) for sc in scs], np.int32)
    lists = [[0, 1], [], [2, 2, 3], [1]]
    for torch_obs in (False, True):
        env = sga.VectorScenarioEnv(scs, timestep=0.1, n=8, terminal_conditions=["max_length"], torch_obs=torch_obs)
        assert not env._lanes_set and tuple(env.reset().shape) == (4, 2, 8, 8)
        assert env.observe_entities_lanes(2, 1)[0].shape[0] == 0 and env._lanes_set  # no observers yet
        env.set_observers(lists)
        for _ in range(6):
            obs, reward, done, info = env.step(np.zeros((4, 2)))
        assert tuple(obs.shape) == (4, 2, 8, 8)
        st = env.engine.state(raw=True)
        trig = trig_of(oracle, st["poses"][..., 3])
        got = env.lane_observation(3, 4, 5.0, 40.0)
        *seen, env_of, slot = env.observe_entities_lanes(2, 2, 20.0)
        if torch_obs:
            assert all(t.is_cuda for t in got) and all(t.is_cuda for t in seen) and env_of.is_cuda and slot.is_cuda
            got, seen = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in seen]
            env_of, slot = env_of.cpu().numpy(), slot.cpu().numpy()
        assert list(env_of) == [i for i, s in enumerate(lists) for _ in s] and list(slot) == [k for s in lists for k in s]
        assert same(got, reference_rows(tabs, net_of, st, trig, np.arange(4), ego, 3, 4, 5.0, 40.0)) and (got[2] > 0).any()
        assert same(seen, reference_rows(tabs, net_of, st, trig, env_of, slot, 2, 2, 20.0, INF))
        env.close()
