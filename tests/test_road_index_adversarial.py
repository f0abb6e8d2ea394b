"""The road cell index (build_road_network, rn_cell_of / rn_ref_point / rn_locate_in_cell / rn_resolve / rn_geoms_at) on
geometry chosen by the index's own structure -- edges on cell lines, vertices on reference points, slivers, holes, degenerate
rings, map coordinates up to 2^40 m, 2 m and 4 m cells, a grid 100,000 cells long (tests/road_shapes.py) -- against exact
answers.  CPU: the oracle's brute force (sgo_geoms_at_points, sgo_surface_contains_points) equals the exact rational
reference on every aimed point.  GPU: sg_road_info_points, sg_road_info, sg_raster_map and ego_off_road equal the oracle on
all of them, through the C ABI."""
import functools

import numpy as np
import pytest

import road_shapes as S
from conftest import bits_equal, load_golden

gpu = pytest.mark.gpu
BITS = (1, 2, 4, 8, 16, 32, 64, 128)
CASES = S.cases()
CASE_IDS = [c[0] for c in CASES]
CASE_NETS = [(cid, name, p, k) for cid, name, p in CASES for k in range(S.N_NETWORKS.get(name, 1))]
N_EXACT_UNIFORM = 2000  # of the uniform class, this many seeded points per network are compared with the exact reference


@functools.lru_cache(maxsize=None)
def _case(name, p):
    nets = S.networks_of(name, p)
    assert len(nets) == S.N_NETWORKS.get(name, 1)
    return nets, S.points_of(name, p, nets)


@functools.lru_cache(maxsize=None)
def _exact(name, p, k):
    """(indices of the points compared exactly, inside [n][P], on a ring [n][P]) of network k of a case: every aimed point and
    N_EXACT_UNIFORM of the uniform ones."""
    nets, pts = _case(name, p)
    xy, cls = pts[k]
    uni = np.nonzero(cls == 0)[0]
    sel = np.sort(np.concatenate([np.nonzero(cls != 0)[0], np.random.default_rng(3).choice(uni, N_EXACT_UNIFORM, replace=False)]))
    return (sel,) + S.contains_exact_many(nets[k], xy[sel], with_on=True)


def _expected_rows(inside, layers, cap):
    """The ABI's outputs for a bool [n][P] matrix: (count, geoms [n][cap] ascending with -1 behind, OR of the layer bits)."""
    n, P = inside.shape
    count = inside.sum(1).astype(np.int32)
    first = np.argsort(~inside, axis=1, kind="stable")[:, :cap]  # the contained polygons first, ascending
    first = np.concatenate([first, np.full((n, max(0, cap - P)), -1)], axis=1).astype(np.int32)
    geoms = np.where(np.arange(cap)[None, :] < count[:, None], first, -1).astype(np.int32)
    lay = np.bitwise_or.reduce(np.where(inside, np.asarray(layers, np.uint32)[None, :], np.uint32(0)), axis=1, initial=0).astype(np.uint32)
    return count, geoms, lay


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("cid,name,p,k", CASE_NETS, ids=[f"{c[0]}-net{c[3]}" for c in CASE_NETS])
def test_oracle_geoms_equal_exact_reference(oracle, cid, name, p, k):
    """oracle.geoms_at_points (count, indices at cap 64 and cap 3, layers) and oracle.surface_contains of every layer bit equal
    the exact rational reference on every point of every aimed class of the network (none skipped) and on N_EXACT_UNIFORM
    seeded points of the uniform class."""
    nets, pts = _case(name, p)
    a, (xy, cls) = nets[k], pts[k]
    sel, inside, _ = _exact(name, p, k)
    assert set(np.nonzero(cls != 0)[0]) <= set(sel) and (cls[sel] == 0).sum() == N_EXACT_UNIFORM
    x, y = xy[sel, 0], xy[sel, 1]
    for cap in (64, 3):
        want = _expected_rows(inside, a["layers"], cap)
        got = oracle.geoms_at_points(a, x, y, cap=cap)
        for w, g, what in zip(want, got, ("count", "geoms", "layers")):
            bad = np.nonzero((w != g).reshape(len(sel), -1).any(1))[0]
            assert len(bad) == 0, (what, cap, len(bad), xy[sel[bad[:5]]].tolist())
    assert np.array_equal(oracle.geoms_at_points(a, x, y, cap=0)[0], inside.sum(1))
    for bit in BITS:
        want = (inside & ((np.asarray(a["layers"]) & bit) != 0)[None, :]).any(1)
        assert np.array_equal(oracle.surface_contains(a, bit, x, y), want), bit
    print(f"{cid} net {k}: {len(sel)} points exact")


def test_oracle_geoms_on_the_fixture(oracle):
    """The oracle reproduces all 13,800 answers of road_info.npz (the reference's own get_geometries_at_point)."""
    from test_road_info import _arrays, _expected, _nets

    g, ri = load_golden("roads"), load_golden("road_info")
    total = 0
    for net in _nets(g):
        a, want, pts = _arrays(g, net), _expected(g, ri, net), g[f"net/{net}/points"]
        count, geoms, layers = oracle.geoms_at_points(a, pts[:, 0], pts[:, 1], cap=48)
        assert count.max() <= 48 and count.tolist() == [len(w) for w in want]
        assert all(list(geoms[i, :count[i]]) == w and (geoms[i, count[i]:] == -1).all() for i, w in enumerate(want))
        assert all(layers[i] == np.bitwise_or.reduce(a["layers"][w], initial=0) for i, w in enumerate(want))
        total += len(pts)
    assert total == 13800


# Lower bounds per (case family, class): (points on a ring, strictly inside something, in nothing) -- half of the smallest
# number the generators give over the placements that keep the lattice (0, 2, 3), by the exact reference; None = the class holds
# no such point there.
_C = {c: i for i, c in enumerate(S.CLASSES)}
MIN_POINTS = {
    "lattice": dict(uniform=(None, 495, 475), vertex=(416, 485, 174), midpoint=(132, 96, 36), on_axis_edge=(396, 285, 109), cell_line=(958, 3278, 1971), sixteenth=(498, 2600, 852), through_vertex=(52, 367, 48), prolongation=(161, 241, 287), outside=(None, None, 49)),
    "traps": dict(uniform=(None, 542, 445), vertex=(41, 105, 10), midpoint=(23, 21, 2), on_axis_edge=(27, 21, 6), cell_line=(90, 2471, 1169), sixteenth=(68, 3018, 433), through_vertex=(24, 56, None), prolongation=(5, 84, 8), outside=(None, None, 49)),
    "thin": dict(uniform=(None, 5, 1990), vertex=(642, 1207, 1893), midpoint=(138, 223, 378), on_axis_edge=(33, None, 33), cell_line=(7, 100, 3864), sixteenth=(3, 530, 3054), through_vertex=(None, None, 1), prolongation=(None, 954, 1491), outside=(None, None, 99)),
    "holes": dict(uniform=(None, 297, 688), vertex=(123, 159, 243), midpoint=(37, 20, 53), on_axis_edge=(61, 6, 55), cell_line=(64, 2242, 3459), sixteenth=(18, 1376, 1410), through_vertex=(2, 20, 1), prolongation=(17, 185, 137), outside=(None, None, 49)),
    "degenerate": dict(uniform=(None, 74, 2917), vertex=(65, 20, 117), midpoint=(27, 2, 25), on_axis_edge=(69, 6, 63), cell_line=(142, 249, 2975), sixteenth=(163, 669, 2762), through_vertex=(1, 12, None), prolongation=(40, 9, 100), outside=(None, None, 148)),
    "stars": dict(uniform=(None, 460, 508), vertex=(141, 566, 141), midpoint=(36, 110, 27), on_axis_edge=(None, None, None), cell_line=(None, 4475, 2199), sixteenth=(None, 2858, 220), through_vertex=(None, None, None), prolongation=(None, 444, 122), outside=(None, None, 49)),
    "square1600": dict(uniform=(None, 457, 543), vertex=(696, 1265, 377), midpoint=(214, 257, 71), on_axis_edge=(516, 368, 148), cell_line=(124, 5933, 3066), sixteenth=(143, 2979, 488), through_vertex=(99, 335, 55), prolongation=(175, 867, 446), outside=(None, None, 49)),
    "square3200": dict(uniform=(None, 428, 571), vertex=(695, 1275, 352), midpoint=(211, 254, 71), on_axis_edge=(516, 359, 156), cell_line=(205, 5696, 3289), sixteenth=(120, 2671, 797), through_vertex=(112, 341, 56), prolongation=(180, 879, 423), outside=(None, None, 49)),
    "strip": dict(uniform=(None, 287, 712), vertex=(114, 195, 17), midpoint=(37, 39, 3), on_axis_edge=(108, 99, 9), cell_line=(726, 2817, 4180), sixteenth=(301, 3043, 425), through_vertex=(10, 80, None), prolongation=(1, 117, 53), outside=(None, None, 49)),
}


@pytest.mark.parametrize("cid,name,p", CASES, ids=CASE_IDS)
def test_point_classes_are_not_empty(cid, name, p):
    """The aimed classes hit what they aim at (exact reference): per family and class at least MIN_POINTS points on a ring,
    strictly inside and in nothing; some point of the lattice and coarse families lies in more than 32 polygons; every trap k
    has reference points 0..k-1 of its cell on its ring and reference point k off it, at every placement."""
    nets, pts = _case(name, p)
    tally = np.zeros((len(S.CLASSES), 3), np.int64)
    most = 0
    for k in range(len(nets)):
        sel, inside, on = _exact(name, p, k)
        cls = pts[k][1][sel]
        for c in range(len(S.CLASSES)):
            m = cls == c
            tally[c] += (on[m].any(1).sum(), inside[m].any(1).sum(), (~inside[m].any(1)).sum())
        most = max(most, int(inside.sum(1).max(initial=0)))
    print(cid, {c: tally[i].tolist() for c, i in _C.items()}, "most polygons at one point:", most)
    assert (tally.sum(1) > 0).all() or name in ("stars", "thin") or p == 1, tally.sum(1)  # (no axis-parallel edges / lattice vertices there)
    assert tally[:, 0].sum() > 0 and tally[:, 1].sum() > 0 and tally[:, 2].sum() > 0
    if p in (None, 0, 2, 3):
        for c, mins in MIN_POINTS[name].items():
            for got, want in zip(tally[_C[c]], mins):
                assert want is None or got >= want, (c, tally[_C[c]].tolist(), mins)
    if name in ("lattice", "square1600", "square3200"):
        assert most == 40
    if name == "traps":
        a = nets[0]
        origin = np.floor(np.asarray(S.PLACEMENTS[p]))
        assert S.grid_of(a)[2] == 1.0 and S.grid_of(a)[0] == np.floor(S.grid_of(a)[0])
        for kk, (ix, iy) in S.trap_cells().items():
            if kk > 7:
                continue
            ref = np.array([(ix + S.REF_FX[s], iy + S.REF_FY[s]) for s in range(8)]) + origin
            _, on = S.contains_exact_many(a, ref, with_on=True)
            assert on[:kk, kk - 1].all() and not on[kk, kk - 1], (kk, on[:, kk - 1])
    if name == "traps" and p == 0:  # k = 8: all eight on the ring
        a = S.traps(None, upto=8)[0]
        ix, iy = S.trap_cells()[8]
        _, on = S.contains_exact_many(a, np.array([(ix + S.REF_FX[s], iy + S.REF_FY[s]) for s in range(8)]), with_on=True)
        assert on[:, 7].all()


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture
def sga():
    import scenario_gym_amd as sga

    return sga


def _ego_batch(xy, E):
    """One scenario per point: the ego (slot 0) stands on it, the other slots in a row beside it."""
    from scenario_gym_amd.engine import DEFAULT_CTRL, PackedScenarios
    from scenario_gym_amd.packing import default_kinds
    from scenario_gym_amd.synthetic import CAR1_BBOX

    R = len(xy)
    kn = np.zeros((R, E, 2, 7))
    kn[:, :, 1, 0] = 1.0
    kn[:, :, :, 1:3] = xy[:, None, None, :]
    kn[:, :, :, 1] += 5.0 * np.arange(E)[None, :, None]
    return PackedScenarios(R, E, np.tile(default_kinds(E, 0), R), np.zeros(R * E, np.int32), np.tile(np.array(CAR1_BBOX), (R * E, 1)),
                           np.arange(R * E + 1, dtype=np.int64) * 2, kn.reshape(-1, 7), np.zeros(R, np.int32), np.zeros(R), np.ones(R),
                           np.tile(DEFAULT_CTRL, (R * E, 1))).validate()


def _scenarios_for(nets, pts, R):
    """Scenario r uses network r % len(nets), the last one none (-1): (net_of [R], all points, their scenario, their network or -1).
    The points of network k go round its scenarios; the first 300 of every network are also asked of the scenario without one."""
    n = len(nets)
    net_of = (np.arange(R) % n).astype(np.int32)
    net_of[R - 1] = -1
    xy, scen, net = [], [], []
    for k, (p, _) in enumerate(pts):
        mine = np.nonzero(net_of == k)[0]
        xy += [p, p[:300]]
        scen += [mine[np.arange(len(p)) % len(mine)], np.full(len(p[:300]), R - 1)]
        net += [np.full(len(p), k), np.full(len(p[:300]), -1)]
    return net_of, np.ascontiguousarray(np.concatenate(xy)), np.concatenate(scen).astype(np.int32), np.concatenate(net)


def _oracle_rows(oracle, nets, xy, net, cap):
    count, layers, geoms = np.zeros(len(xy), np.int32), np.zeros(len(xy), np.uint32), np.full((len(xy), cap), -1, np.int32)
    for k, a in enumerate(nets):
        m = net == k
        count[m], geoms[m], layers[m] = oracle.geoms_at_points(a, xy[m, 0], xy[m, 1], cap=cap)
    return count, geoms, layers


@gpu
@pytest.mark.parametrize("cid,name,p", CASES, ids=CASE_IDS)
def test_points_equal_oracle(sga, oracle, cid, name, p):
    """sg_road_info_points on every point of every class of every network of the case (several networks on one handle, the
    scenarios alternating over them, one scenario without a network): count, the first cap indices, the -1 tail and layers are
    the oracle's, 0 mismatches, at cap = 32, cap = 3 and cap = 0 with NULL geoms."""
    nets, pts = _case(name, p)
    R = 2 * len(nets) + 1
    net_of, xy, scen, net = _scenarios_for(nets, pts, R)
    eng = sga.RolloutEngine(R, 4, timestep=0.1)
    eng.upload(_ego_batch(np.zeros((R, 2)), 4))
    eng.set_road_networks(nets, net_of)
    n = len(xy)
    for cap in (32, 3, 0):
        count, layers, geoms = np.full(n, -7, np.int32), np.full(n, 77, np.uint32), np.full((n, cap), -7, np.int32)
        rc = eng.lib.sg_road_info_points(eng.h, n, scen.ctypes.data, xy.ctypes.data, cap, count.ctypes.data,
                                         geoms.ctypes.data if cap else None, layers.ctypes.data)
        assert rc == 0, eng.lib.sg_last_error(eng.h)
        oc, og, ol = _oracle_rows(oracle, nets, xy, net, cap)
        bad = np.nonzero((count != oc) | (layers != ol) | (geoms != og).any(1))[0]
        assert len(bad) == 0, (cap, len(bad), xy[bad[:5]].tolist(), count[bad[:5]], oc[bad[:5]])
    assert (oc[net < 0] == 0).all() and (oc > 0).any() == any(len(a["layers"]) for a in nets)
    eng.close()
    print(f"{cid}: {n} points x 3 capacities, 0 mismatches")


def _ego_points(pts):
    """The points sg_upload takes as knots: finite and below 1e16 in magnitude."""
    return [(xy[(np.abs(xy) < 1e16).all(1)], None) for xy, _ in pts]


def _entities_agree(sga, oracle, nets, pts, E, chunk):
    total = 0
    for k, (p, _) in enumerate(_ego_points(pts)):
        for a0 in range(0, len(p), chunk):
            xy = np.concatenate([p[a0:a0 + chunk], p[a0:a0 + 1]])  # (one more scenario, without a network)
            R = len(xy)
            net_of = np.zeros(R, np.int32)
            net_of[R - 1] = -1
            eng = sga.RolloutEngine(R, E, timestep=0.1)
            eng.upload(_ego_batch(xy, E))
            eng.set_road_networks([nets[k]], net_of)
            st = eng.state()
            assert st["present"][:, 0].all()
            pos = np.ascontiguousarray(st["poses"][:, 0, :2])
            assert bits_equal(pos, xy)
            count, geoms, layers = (np.full((R, E), -7, np.int32), np.full((R, E, 32), -7, np.int32), np.full((R, E), 77, np.uint32))
            assert eng.lib.sg_road_info(eng.h, 32, count.ctypes.data, geoms.ctypes.data, layers.ctypes.data, 0) == 0
            oc, og, ol = oracle.geoms_at_points(nets[k], pos[:, 0], pos[:, 1], cap=32)
            oc[R - 1], og[R - 1], ol[R - 1] = 0, -1, 0
            bad = np.nonzero((count[:, 0] != oc) | (layers[:, 0] != ol) | (geoms[:, 0] != og).any(1))[0]
            assert len(bad) == 0, ("sg_road_info", len(bad), pos[bad[:5]].tolist())
            # the other slots: the oracle at their own poses
            others = st["poses"][:, 1:, :2].reshape(-1, 2)
            oc2 = oracle.geoms_at_points(nets[k], others[:, 0], others[:, 1], cap=0)[0].reshape(R, E - 1)
            oc2[R - 1] = 0
            assert np.array_equal(count[:, 1:], oc2)
            maps = eng.raster_map(list(BITS), 0.0, 0.0, 1, 1)[:, :, 0, 0]
            flags = eng.terminal_flags()
            for j, bit in enumerate(BITS):
                want = oracle.surface_contains(nets[k], bit, pos[:, 0], pos[:, 1])
                want[R - 1] = False
                assert np.array_equal(maps[:, j], want), ("sg_raster_map", bit, pos[np.nonzero(maps[:, j] != want)[0][:5]].tolist())
                if bit == 1:
                    assert np.array_equal((flags & 8) == 0, want), ("ego_off_road", pos[np.nonzero(((flags & 8) == 0) != want)[0][:5]].tolist())
            eng.close()
            total += R - 1
    return total


@gpu
@pytest.mark.parametrize("E", [4, 64])
@pytest.mark.parametrize("cid,name,p", CASES, ids=CASE_IDS)
def test_entities_and_layer_kernels_agree_with_oracle(sga, oracle, cid, name, p, E):
    """The same points as ego poses, one scenario per point (the poses compared are those state() reads back; the points
    sg_upload need not take -- not finite, 1e300 -- stay with the point query): sg_road_info of every slot equals the oracle;
    every surface layer of raster_map(bits, 0, 0, 1, 1) and the ego_off_road bit of terminal_flags equal
    oracle.surface_contains per bit -- rn_resolve with every `want` mask on the adversarial cells; the last scenario of every
    upload has no network and answers nothing.  4 and 64 entity slots."""
    nets, pts = _case(name, p)
    n = _entities_agree(sga, oracle, nets, pts, E, 16384)
    print(f"{cid} E={E}: {n} ego poses x (sg_road_info, 8 raster layers, ego_off_road), 0 mismatches")


@gpu
@pytest.mark.parametrize("E", [300, 600])
def test_entities_and_layer_kernels_agree_with_oracle_wide(sga, oracle, E):
    """The lattice family at the origin on 300 and 600 entity slots per scenario (several wavefronts, the multi-kernel step)."""
    nets, pts = _case("lattice", 0)
    n = _entities_agree(sga, oracle, nets, pts, E, 2048)
    print(f"lattice-p0 E={E}: {n} ego poses, 0 mismatches")


@gpu
def test_refusals_are_loud(sga, oracle):
    """A polygon through all eight reference points of a cell, and 70,000 edges of one polygon in one cell: sg_set_road_networks
    returns SG_ERR_INVALID and sg_last_error names the network and the reason.  What the handle answers afterwards:
    sg_set_road_networks drops the networks it had BEFORE it builds the new index, so after a refusal the handle has none --
    every count is 0, no layer bit, rasters empty, every ego off the road -- until the next successful call, which is answered
    as if the refusal had not happened."""
    good = S.lattice(np.random.default_rng(1))[0]
    R = 4
    xy = np.ascontiguousarray(np.tile([[30.0, 30.0], [30.25, 30.0]], (R, 1))[:R])
    scen = np.arange(R, dtype=np.int32)
    eng = sga.RolloutEngine(R, 4, timestep=0.1)
    eng.upload(_ego_batch(xy, 4))
    eng.set_road_networks([good], np.zeros(R, np.int32))
    before = eng.road_info_points(scen, xy, cap=64)
    assert before[0].tolist() == oracle.geoms_at_points(good, xy[:, 0], xy[:, 1], cap=64)[0].tolist() and before[0].max() == 40
    for bad, why in ((S.traps(None, upto=8)[0], b"reference points all lie on a polygon boundary"),
                     (S.circle(70000), b"more than 65535 edges of one polygon in one cell")):
        with pytest.raises(RuntimeError):
            eng.set_road_networks([good, bad], np.zeros(R, np.int32))
        msg = eng.lib.sg_last_error(eng.h)
        assert b"sg_set_road_networks: network 1 cannot be indexed" in msg and why in msg, msg
        c, g, l = eng.road_info_points(scen, xy, cap=8)
        assert not c.any() and (g == -1).all() and not l.any()
        ce, ge, le = eng.road_info(cap=8)
        assert not ce.any() and (ge == -1).all() and not le.any()
        assert not eng.raster_map(list(BITS), 0.0, 0.0, 1, 1).any() and (eng.terminal_flags() & 8).all()
        eng.set_road_networks([good], np.zeros(R, np.int32))
        after = eng.road_info_points(scen, xy, cap=64)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
    eng.close()


def _far_crowd(which):
    """make_crowd_roads' building blocks and crowd: translated to (4.5e5, 5.4e6) ('far'), or with two small polygons 3.2 km
    apart added to the network, which makes the builder's cells 4 m wide ('coarse')."""
    from scenario_gym_amd import synthetic

    R, E, steps = 4, 64, 200
    packed, net, net_of = synthetic.make_crowd_roads(R, E, n_steps=steps, side=30.0, blocks=2, building=10.0)
    net = {k: np.array(net[k]) for k in ("ring_off", "vert_off", "verts", "layers")}
    net["verts"] = np.asarray(net["verts"], np.float64).reshape(-1, 2)
    if which == "far":
        off = np.array(S.PLACEMENTS[2])
        packed.knots[:, 1:3] += off
        packed.routes += off
        net["verts"] = net["verts"] + off
    else:
        extra = np.array(S._rect(-1600, -1600, -1599, -1599) + S._rect(1599, 1599, 1600, 1600), np.float64)
        net = dict(ring_off=np.concatenate([net["ring_off"], net["ring_off"][-1] + [1, 2]]),
                   vert_off=np.concatenate([net["vert_off"], net["vert_off"][-1] + [4, 8]]),
                   verts=np.concatenate([net["verts"], extra]), layers=np.concatenate([net["layers"], [1, 32]]).astype(np.uint32))
        assert S.grid_of(net)[2] == 4.0
    net_of = np.array(net_of, np.int32)
    net_of[2] = -1
    return packed.validate(), net, net_of, steps


@gpu
@pytest.mark.parametrize("which", ["far", "coarse"])
def test_crowd_boundary_phase_on_coarse_and_far_networks(sga, oracle, monkeypatch, which):
    """A crowd of 64 between buildings at map coordinates (4.5e5, 5.4e6) -- the filter margin of ped_boundary_terms grows with
    the largest coordinate -- and on a network 3.2 km wide (4 m cells): the crowd kernel equals the oracle bit for bit
    (verify_engine with the network) and the general pedestrian kernel (SG_CROWD_ROADS=0) bit for bit; the scenario without
    a network walks as if there were none."""
    from oracle import check

    packed, net, net_of, steps = _far_crowd(which)
    R, E, dt = packed.n_scenarios, packed.n_entities, 1 / 30
    out = []
    for roads in ("1", "0", "off"):
        monkeypatch.setenv("SG_CROWD_ROADS", "0" if roads == "0" else "1")
        eng = sga.RolloutEngine(R, E, timestep=dt, terminal_conditions=["max_length"], event_capacity=256)
        eng.upload(packed)
        if roads != "off":
            eng.set_road_networks([net], net_of)
        eng.rollout(steps)
        out.append((eng.state(), eng.metrics()))
        if roads == "1":
            ver = check.verify_engine(eng, packed, dt, steps, K=R, event_cap=256, ped=True, road_of=lambda r: net if net_of[r] == 0 else None)
            assert ver["equal"], ver["mismatches"]
        eng.close()
    (sa, (ra, ea)), (sb, (rb, eb)), (sc, _) = out
    for k in ("poses", "vels", "dists", "force", "ctrl_state", "present"):
        assert bits_equal(sa[k], sb[k]), k
    assert np.array_equal(sa["coll"], sb["coll"]) and ra.tobytes() == rb.tobytes() and ea.tobytes() == eb.tobytes()
    assert bits_equal(sa["poses"][2], sc["poses"][2]) and not bits_equal(sa["poses"][0], sc["poses"][0])  # the network is felt
