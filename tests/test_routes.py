"""Routes and the route / recorded-track observation: sg_set_routes / sg_route_observation / sg_route_observation_observers
(route_observation_kernel) and the Python layers over them.

The yardstick is route_reference: the definition in include/sgym.h at sg_route_observation restated in numpy -- np.where for the
selects, two products and a sum per dot product, a sequential Python sum for cum -- with every sine and cosine from oracle.sincos and
the recorded pose from oracle.position_at_t(knots, t, 0, 0).  The device must equal it bit for bit on feat and exactly on info.

CPU  hand-made scenes with exact answers; dense sampling of the polyline as an independent bound on the distance; the scenes of
     route_scenes.batch held to their purpose; the C surface
GPU  1. the batch scenes at E = 3, 65, 100, 600: after the reset, after ten steps of sg_step_drivers, after sg_reset_scenarios on half
        the batch; n_ahead 0, 1, 16, spacing 0 and 2; host and device outputs, info NULL, every byte written
     2. lifetime and refusals
     3. VectorScenarioEnv(drivers=..., driver_progress=1.0); State.route_observation and the environment's route calls
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import policy_scenes as PS
import route_scenes as RS
from test_drivers import _bits, _scenario_objects

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float64
NFEAT, NINFO, MAX_AHEAD = 11, 2, 16


@pytest.fixture(scope="module")
def sga():
    import scenario_gym_amd as sga

    return sga


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def route_rows(path):
    """The rows sg_set_routes builds for one polyline, as arrays over its segments, and total."""
    path = np.asarray(path, F).reshape(-1, 2)
    a, b = path[:-1], path[1:]
    ex, ey = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    L2 = ex * ex + ey * ey
    ln = np.sqrt(L2)
    cum, run = np.zeros(len(ln)), F(0.0)
    for i in range(len(ln)):
        cum[i] = run
        run = run + ln[i]
    total = cum[-1] + ln[-1] if len(ln) else F(0.0)
    return dict(ax=a[:, 0], ay=a[:, 1], bx=b[:, 0], by=b[:, 1], ex=ex, ey=ey, L2=L2, len=ln, cum=cum, total=total, n=len(ln))


def project(g, px, py):
    """The point-to-segment rule of sg_lane_observation on every row: (d2, dx, dy, t)."""
    wx, wy = px - g["ax"], py - g["ay"]
    t = (wx * g["ex"] + wy * g["ey"]) / g["L2"]
    at_a = (g["L2"] == 0.0) | ~(t > 0.0)
    at_b = ~at_a & (t >= 1.0)
    cx = np.where(at_a, g["ax"], np.where(at_b, g["bx"], g["ax"] + t * g["ex"]))
    cy = np.where(at_a, g["ay"], np.where(at_b, g["by"], g["ay"] + t * g["ey"]))
    t = np.where(at_a, 0.0, np.where(at_b, 1.0, t))
    dx, dy = px - cx, py - cy
    return dx * dx + dy * dy, dx, dy, t


def route_one(oracle, pose, present, t, knots, path, n_ahead, spacing):
    """One observer: (feat [NFEAT + 2 * n_ahead], info [2])."""
    feat, info = np.zeros(NFEAT + 2 * n_ahead), np.array([-1, -1], np.int32)
    if not present:
        return feat, info
    px, py = F(pose[0]), F(pose[1])
    s, c = (F(q) for q in oracle.sincos(pose[3]))
    # the recorded track
    if len(knots) == 0:
        info[1] = 2
    else:
        rec = oracle.position_at_t(knots, t, 0, 0)
        X, Y = F(rec[0]) - px, F(rec[1]) - py
        sr, cr = (F(q) for q in oracle.sincos(rec[3]))
        feat[0], feat[1] = X * c + Y * s, Y * c - X * s
        feat[2] = np.sqrt(X * X + Y * Y)
        feat[3], feat[4] = cr * c + sr * s, sr * c - cr * s
        info[1] = -1 if t < knots[0, 0] else 1 if t > knots[-1, 0] else 0
    # the route
    if path is None:
        return feat, info
    g = route_rows(path)
    if g["n"] == 0:
        return feat, info
    d2, dx, dy, ts = project(g, px, py)
    cand = np.where(np.isfinite(d2), d2, np.inf)
    if not np.isfinite(cand).any():
        return feat, info
    b = int(np.argmin(cand))  # (the first of equal minima: the lower index)
    ln = g["len"][b]
    ux, uy = (g["ex"][b] / ln, g["ey"][b] / ln) if ln != 0.0 else (F(0.0), F(0.0))
    s0 = g["cum"][b] + ts[b] * ln
    feat[5] = ux * dy[b] - uy * dx[b]
    feat[6], feat[7] = c * ux + s * uy, s * ux - c * uy
    feat[8], feat[9], feat[10] = s0, g["total"] - s0, np.sqrt(d2[b])
    info[0] = b
    # the look-ahead
    for m in range(1, n_ahead + 1):
        target = s0 + F(m) * F(spacing)
        if target > g["total"]:
            x, y = g["bx"][-1], g["by"][-1]
        else:
            q = int(np.searchsorted(g["cum"], target, "right")) - 1  # the last segment with cum <= target
            u = (target - g["cum"][q]) / g["len"][q] if g["len"][q] != 0.0 else F(0.0)
            x, y = (g["bx"][q], g["by"][q]) if u >= 1.0 else (g["ax"][q] + u * g["ex"][q], g["ay"][q] + u * g["ey"][q])
        X, Y = x - px, y - py
        feat[11 + 2 * (m - 1)], feat[12 + 2 * (m - 1)] = X * c + Y * s, Y * c - X * s
    return feat, info


def route_reference(oracle, st, scs, scen, slot, routes, n_ahead, spacing):
    """The definition for the observers (scen[j], slot[j]) on a batch state as RolloutEngine.state(raw=True) gives it (poses, present,
    t); routes: {(scenario, slot): path}.  Returns (feat [n, NFEAT + 2 * n_ahead], info [n, 2] int32)."""
    n = len(scen)
    feat, info = np.zeros((n, NFEAT + 2 * n_ahead)), np.zeros((n, NINFO), np.int32)
    with np.errstate(all="ignore"):
        for j in range(n):
            r, k = int(scen[j]), int(slot[j])
            sc = scs[r]
            knots = sc["knots"][sc["knot_off"][k]:sc["knot_off"][k + 1]]
            feat[j], info[j] = route_one(oracle, st["poses"][r, k], st["present"][r, k], float(st["t"][r]), knots, routes.get((r, k)),
                                         n_ahead, spacing)
    return feat, info


def same(got, want):
    """feat bit for bit, info exactly."""
    return (got[0].shape == want[0].shape and np.array_equal(_bits(np.asarray(got[0])), _bits(want[0])) and
            np.array_equal(np.asarray(got[1]), want[1]))


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def _hand(oracle, name, t=0.0):
    sc = RS.hand()[name]
    x, y, h = sc["pose"]
    knots = PS._still(x, y, h)
    pose = np.array([x, y, 0.0, h, 0.0, 0.0])
    with np.errstate(all="ignore"):
        return route_one(oracle, pose, True, t, knots, sc["path"], sc["n_ahead"], sc["spacing"])


def test_hand_made_scenes_have_their_exact_answers(oracle):
    # 3 beyond the end of an axis-parallel route and 4 to its left: 5 from its last point
    feat, info = _hand(oracle, "offset345")
    assert info.tolist() == [0, 0] and feat[10] == 5.0 and feat[5] == 4.0 and feat[8] == 10.0 and feat[9] == 0.0
    assert (feat[:5] == [0.0, 0.0, 0.0, 1.0, 0.0]).all()  # on its recording, heading as recorded
    feat, info = _hand(oracle, "left4")
    assert info[0] == 0 and feat[5] == 4.0 and feat[6] == 1.0 and feat[7] == 0.0 and feat[8] == 4.0 and feat[9] == 16.0 and feat[10] == 4.0
    assert feat[11:].tolist() == [3.0, -4.0, 6.0, -4.0]  # 7 and 10 along the axis, seen from (4, 4)
    # on a shared vertex, and beside it with both segments clamped to it: the lower index
    feat, info = _hand(oracle, "vertex")
    assert info[0] == 0 and feat[10] == 0.0 and feat[8] == 10.0 and feat[9] == 10.0
    feat, info = _hand(oracle, "shared")
    g = route_rows(RS.hand()["shared"]["path"])
    d2 = project(g, F(12.0), F(-2.0))[0]
    assert d2[0] == d2[1] == 8.0 and info[0] == 0 and feat[8] == 10.0
    # zero-length segments in the middle and at the end: never the best while a proper one ties, and walked through by the look-ahead
    feat, info = _hand(oracle, "zero_len")
    g = route_rows(RS.hand()["zero_len"]["path"])
    assert g["len"].tolist() == [4.0, 0.0, 8.0, 0.0] and g["cum"].tolist() == [0.0, 4.0, 4.0, 12.0] and g["total"] == 12.0
    assert info[0] == 2 and feat[8] == 6.0 and feat[9] == 6.0 and feat[10] == 1.0
    assert feat[11:].tolist() == [2.0, -1.0, 4.0, -1.0, 6.0, -1.0, 6.0, -1.0]  # 8, 10, 12 (== total: the last row, u = 0), 14 (beyond)
    # a target equal to a cum value starts the next segment; a target equal to total is its end; then beyond
    feat, info = _hand(oracle, "on_cum")
    assert info[0] == 0 and feat[8] == 2.0 and feat[9] == 10.0
    assert feat[11:].tolist() == [2.0, -1.0, 2.0, 1.0, 2.0, 3.0, 2.0, 5.0, 2.0, 7.0]  # s = 4 (the corner), 6, 8, 10, 12 (the end)
    feat, info = _hand(oracle, "beyond")
    assert feat[8] == 8.0 and feat[11:].tolist() == [8.0, 1.0, 12.0, 1.0, 12.0, 1.0]  # 16, then 24 and 32 beyond total = 20: the last point
    # facing against the route
    feat, info = _hand(oracle, "against")
    assert feat[6] == -1.0 and feat[5] == 0.5 and abs(feat[7]) < 1e-15 and feat[8] == 5.0
    assert feat[11] == -2.0  # the point ahead on the route lies behind the observer


def test_track_part_by_hand(oracle):
    """The recording against hand-made poses: before, within and after the knots, a single knot, no knots, and an absent observer."""
    knots = PS._along([(0.0, 0.0), (10.0, 0.0), (10.0, 10.0)], 5.0, t0=1.0)  # knots at t = 1, 3, 5; heading 0 then pi / 2
    pose = np.array([3.0, 4.0, 0.0, 0.0, 0.0, 0.0])
    one = lambda t, k=knots, present=True: route_one(oracle, pose, present, t, k, None, 2, 1.0)  # noqa: E731
    feat, info = one(0.5)
    assert info.tolist() == [-1, -1] and feat[:5].tolist() == [-3.0, -4.0, 5.0, 1.0, 0.0] and not feat[5:].any()
    feat, info = one(2.0)  # half way along the first segment: (5, 0)
    assert info.tolist() == [-1, 0] and feat[:3].tolist() == [2.0, -4.0, np.sqrt(F(20.0))]
    feat, info = one(7.0)
    assert info.tolist() == [-1, 1] and feat[:2].tolist() == [7.0, 6.0] and abs(feat[3]) < 1e-15 and feat[4] == 1.0
    feat, info = one(1.0, knots[:1])
    assert info.tolist() == [-1, 0] and feat[:3].tolist() == [-3.0, -4.0, 5.0]
    feat, info = one(1.0, knots[:0])
    assert info.tolist() == [-1, 2] and not feat.any()
    feat, info = one(2.0, present=False)
    assert info.tolist() == [-1, -1] and not feat.any()


@pytest.mark.parametrize("role", ["r3", "r65", "r130", "late"])
def test_distance_is_bounded_by_dense_sampling(oracle, role):
    """An independent method: the distance to the nearest of 1 cm samples of the polyline bounds feat[10] from above, within the
    sampling step."""
    cfg = RS.batch(65)
    r, k = cfg["who"][role]
    path = cfg["routes"][(r, k)]
    sc = cfg["scs"][r]
    first = sc["knots"][sc["knot_off"][k]]
    pose = np.array([first[1] + 0.4, first[2] - 0.3, 0.0, first[4], 0.0, 0.0])
    feat, info = route_one(oracle, pose, True, 0.0, sc["knots"][sc["knot_off"][k]:sc["knot_off"][k + 1]], path, 0, 0.0)
    step = 0.01
    pts = []
    for a, b in zip(path[:-1], path[1:]):
        n = max(int(np.ceil(np.hypot(*(b - a)) / step)), 1)
        pts.append(a + (b - a) * np.linspace(0.0, 1.0, n + 1)[:, None])
    pts = np.concatenate(pts)
    sampled = np.hypot(pts[:, 0] - pose[0], pts[:, 1] - pose[1]).min()
    assert info[0] >= 0 and feat[10] <= sampled + 1e-12 and sampled - feat[10] <= step


@pytest.mark.parametrize("E", [3, 65, 100, 600])
def test_batch_scenes_hold_every_case(oracle, E):
    """What the device comparison is meant to cover is in the scenes, judged by the yardstick on the hand-made reset state."""
    cfg = RS.batch(E)
    scs, who = cfg["scs"], cfg["who"]
    assert sorted(len(p) for p in cfg["routes"].values())[:4] == [0, 1, 2, 2] and {3, 64, 65, 66, 130} <= {len(p) for p in cfg["routes"].values()}
    assert len({(r, k) for r, k in who.values()}) == len(RS.ROLES) and who["none"] not in cfg["routes"]
    poses, present = np.zeros((4, E, 6)), np.zeros((4, E), bool)
    for r, sc in enumerate(scs):
        first = sc["knots"][sc["knot_off"][:-1]]
        poses[r], present[r] = first[:, 1:], first[:, 0] <= 0.0
    st = dict(poses=poses, present=present, t=np.zeros(4))
    feat, info = route_reference(oracle, st, scs, cfg["obs_scen"], cfg["obs_slot"], cfg["routes"], 2, 2.0)
    by = {role: j for j, role in enumerate(RS.ROLES)}
    for role, seg in RS.BESIDE.items():
        assert info[by[role], 0] == seg, role  # r65: the last lane of the first block; r66, r130: the second block
    assert info[by["r0"], 0] == info[by["r1"], 0] == info[by["none"], 0] == -1 and info[by["r2"], 0] == 0
    assert info[by["late"]].tolist() == [-1, -1] and not feat[by["late"]].any() and not present[who["late"]]
    k = who["single"]
    assert scs[k[0]]["knot_off"][k[1] + 1] - scs[k[0]]["knot_off"][k[1]] == 1 and info[by["single"]].tolist() == [0, 0]
    # observers in every 64-slot block, the egos, an absent filler, duplicates
    blocks = {int(s) // 64 for s in cfg["obs_slot"]}
    assert blocks == set(range((E + 63) // 64))
    pairs = list(zip(cfg["obs_scen"].tolist(), cfg["obs_slot"].tolist()))
    assert all((r, scs[r]["ego"]) in pairs for r in range(4)) and pairs[-2:] == pairs[:2]
    assert E == 3 or any(not present[r, s] and (r, s) != who["late"] for r, s in pairs)  # (no fillers at E == 3: "late" alone)
    assert np.isfinite(feat).all()


NEW_SYMBOLS = ("sg_set_routes", "sg_route_observation", "sg_route_observation_observers")


def test_abi_declares_the_route_calls():
    """include/sgym.h declares the three calls and the SG_RT_* values, _lib.SYMBOLS names them, the built library exports them, and
    the ABI version is still 7 (the calls are additions)."""
    import scenario_gym_amd._lib as L

    header = open(os.path.join(ROOT, "include", "sgym.h")).read()
    assert L.ABI_VERSION == 7 and re.search(r"#define SG_ABI_VERSION 7\b", header)
    for name, value in dict(SG_ROUTE_MAX_AHEAD=16, SG_RT_NINFO=2, SG_RT_NFEAT=11).items():
        assert re.search(r"#define %s\s+%d\b" % (name, value), header), name
    assert (L.ROUTE_MAX_AHEAD, L.RT_NINFO, L.RT_NFEAT) == (MAX_AHEAD, NINFO, NFEAT)
    assert re.search(r"\bint sg_set_routes\(sg_handle \*h, int64_t n, const int32_t \*scenario, const int32_t \*slot, const int64_t \*pt_off, "
                     r"const double \*pts\);", header)
    for name in NEW_SYMBOLS[1:]:
        assert re.search(r"\bint " + name + r"\(sg_handle \*h, int32_t n_ahead, double spacing, double \*feat, int32_t \*info, "
                         r"int32_t outputs_device\);", header), name
    lib = C.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and hasattr(lib, name), name


# ---------------------------------------------------------------------------------------------------------------------------- GPU
TERMS = ["max_length"]


def _engine(sga, cfg):
    scs = cfg["scs"]
    eng = sga.RolloutEngine(len(scs), len(scs[0]["etype"]), timestep=PS.DT, terminal_conditions=TERMS, event_capacity=16)
    eng.upload(PS.pack(scs))
    eng.set_drivers(cfg["drv_scen"], cfg["drv_slot"])
    return eng


def _check_all_outputs(eng, oracle, cfg, what):
    """Every look-ahead setting, for the observer list and the egos, host and device outputs; then the optional array left out and
    every byte written."""
    import torch

    scs = cfg["scs"]
    R = len(scs)
    st = eng.state(raw=True)
    ego_scen, ego_slot = np.arange(R, dtype=np.int32), np.array([sc["ego"] for sc in scs], np.int32)
    pairs = list(zip(cfg["obs_scen"].tolist(), cfg["obs_slot"].tolist()))
    for n_ahead, spacing in ((0, 0.0), (1, 2.0), (16, 2.0), (16, 0.0)):
        want = route_reference(oracle, st, scs, cfg["obs_scen"], cfg["obs_slot"], cfg["routes"], n_ahead, spacing)
        got = eng.route_observation(n_ahead, spacing, observers=True)
        assert same(got, want), (what, n_ahead, spacing)
        dev = eng.route_observation(n_ahead, spacing, observers=True, device=True)
        assert same([t.cpu().numpy() for t in dev], want), (what, n_ahead, spacing, "device")
        want_ego = route_reference(oracle, st, scs, ego_scen, ego_slot, cfg["routes"], n_ahead, spacing)
        got_ego = eng.route_observation(n_ahead, spacing)
        assert same(got_ego, want_ego), (what, n_ahead, spacing, "egos")
        for r in range(R):  # the observer (r, ego of r) gets the bytes of the ego call; duplicates each get their rows
            j = pairs.index((r, int(ego_slot[r])))
            assert got[0][j].tobytes() == got_ego[0][r].tobytes() and got[1][j].tobytes() == got_ego[1][r].tobytes()
        assert got[0][-2:].tobytes() == got[0][:2].tobytes() and got[1][-2:].tobytes() == got[1][:2].tobytes()
    # info == NULL, and every byte of the arrays given written (pre-filled with 0xA5; guard words behind them untouched)
    n, W = len(pairs), NFEAT + 2 * 3
    want = route_reference(oracle, st, scs, cfg["obs_scen"], cfg["obs_slot"], cfg["routes"], 3, 1.5)
    buf = np.full(n * W * 8 + 32, 0xA5, np.uint8)
    ibuf = np.full(n * NINFO * 4 + 32, 0xA5, np.uint8)
    assert eng.lib.sg_route_observation_observers(eng.h, 3, 1.5, buf.ctypes.data, None, 0) == 0
    assert buf[:n * W * 8].tobytes() == want[0].tobytes() and (buf[n * W * 8:] == 0xA5).all()
    buf[:] = 0xA5
    assert eng.lib.sg_route_observation_observers(eng.h, 3, 1.5, buf.ctypes.data, ibuf.ctypes.data, 0) == 0
    assert buf[:n * W * 8].tobytes() == want[0].tobytes() and (buf[n * W * 8:] == 0xA5).all()
    assert ibuf[:n * NINFO * 4].tobytes() == want[1].tobytes() and (ibuf[n * NINFO * 4:] == 0xA5).all()
    t = torch.full((n * W * 8 + 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ti = torch.full((n * NINFO * 4 + 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert eng.lib.sg_route_observation_observers(eng.h, 3, 1.5, t.data_ptr(), None, 1) == 0
    eng.synchronize()
    assert t.cpu().numpy()[:n * W * 8].tobytes() == want[0].tobytes() and (t.cpu().numpy()[n * W * 8:] == 0xA5).all()
    t.fill_(0xA5)
    torch.cuda.synchronize()
    assert eng.lib.sg_route_observation_observers(eng.h, 3, 1.5, t.data_ptr(), ti.data_ptr(), 1) == 0
    eng.synchronize()
    assert t.cpu().numpy()[:n * W * 8].tobytes() == want[0].tobytes() and (t.cpu().numpy()[n * W * 8:] == 0xA5).all()
    assert ti.cpu().numpy()[:n * NINFO * 4].tobytes() == want[1].tobytes() and (ti.cpu().numpy()[n * NINFO * 4:] == 0xA5).all()
    return st, want


# --------------------------------------------------------------------------------------------------------- 1. against the yardstick
@gpu
@pytest.mark.parametrize("E", [3, 65, 100, 600])
def test_route_observation_against_the_yardstick(sga, oracle, E):
    """The batch scenes after the reset, after ten steps of sg_step_drivers with steering (the poses leave the recordings, t falls
    between knots) and after sg_reset_scenarios on half the batch; the cases of the scenes are checked on the device's own state."""
    cfg = RS.batch(E)
    scs, who = cfg["scs"], cfg["who"]
    by = {role: j for j, role in enumerate(RS.ROLES)}
    eng = _engine(sga, cfg)
    eng.set_observers(cfg["obs_scen"], cfg["obs_slot"])
    # without sg_set_routes the call succeeds: the track part, and -1 / zeros for the route
    bare = eng.route_observation(2, 2.0, observers=True)
    assert same(bare, route_reference(oracle, eng.state(raw=True), scs, cfg["obs_scen"], cfg["obs_slot"], {}, 2, 2.0))
    assert (bare[1][:, 0] == -1).all() and not bare[0][:, 5:].any() and bare[0][:, :5].any()
    eng.set_routes(*RS.route_lists(cfg["routes"]))
    st, want = _check_all_outputs(eng, oracle, cfg, "reset")
    for role, seg in RS.BESIDE.items():
        assert want[1][by[role], 0] == seg, role
    assert not st["present"][who["late"]] and want[1][by["late"]].tolist() == [-1, -1]
    assert st["present"][who["single"]] and want[1][by["single"]].tolist() == [0, 0]
    eng.step_drivers(cfg["actions"], RS.STEPS)
    st, want = _check_all_outputs(eng, oracle, cfg, "stepped")
    assert st["present"][who["late"]] and want[1][by["late"], 1] == -1 and want[1][by["late"], 0] >= 0  # in the scene before its first knot
    assert st["present"][who["short"]] and want[1][by["short"], 1] == 1                                  # ... and after its last
    assert want[1][by["single"], 1] == (1 if st["present"][who["single"]] else -1)  # (it stays in the scene where it is the ego: a replay agent)
    assert (want[0][[by[q] for q in ("r3", "r64", "r65", "r66", "short")], 2] > 0.05).all()               # the drivers left their recordings
    assert (want[1][:len(RS.ROLES), 1] == 0).sum() >= 6 and want[0][by["r130"], 8] > 0.0
    eng.reset_scenarios(np.array([1, 0, 1, 0], np.uint8))
    st, _ = _check_all_outputs(eng, oracle, cfg, "half reset")
    assert st["t"][0] == 0.0 and st["t"][1] > 0.5
    eng.close()


# ------------------------------------------------------------------------------------------------------ 2. lifetime and refusals
@gpu
def test_lifetime_and_refusals(sga, oracle):
    INVALID, STATE = -1, -3
    cfg = RS.batch(65)
    scs = cfg["scs"]
    packed = PS.pack(scs)
    eng = sga.RolloutEngine(4, 65, timestep=PS.DT, terminal_conditions=TERMS, event_capacity=16)
    lib, h = eng.lib, eng.h
    scen, slot, paths = RS.route_lists(cfg["routes"])
    n = len(scen)

    def arrays(paths, pt_off=None):
        off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64) if pt_off is None else np.ascontiguousarray(pt_off, np.int64)
        pts = np.ascontiguousarray(np.concatenate([np.asarray(p, F).reshape(-1, 2) for p in paths]))
        return off, pts

    def call(scen=scen, slot=slot, paths=paths, pt_off=None, n_=None, null=()):
        scen, slot = np.ascontiguousarray(scen, np.int32), np.ascontiguousarray(slot, np.int32)
        off, pts = arrays(paths, pt_off)
        ptr = dict(scenario=scen.ctypes.data, slot=slot.ctypes.data, pt_off=off.ctypes.data, pts=pts.ctypes.data)
        for name in null:
            ptr[name] = None
        return lib.sg_set_routes(h, len(scen) if n_ is None else n_, ptr["scenario"], ptr["slot"], ptr["pt_off"], ptr["pts"])

    feat = np.zeros((4, NFEAT))
    assert call() == STATE and lib.sg_route_observation(h, 0, 0.0, feat.ctypes.data, None, 0) == STATE  # before sg_upload
    assert lib.sg_route_observation_observers(h, 0, 0.0, feat.ctypes.data, None, 0) == STATE
    eng.upload(packed)
    eng.set_drivers(cfg["drv_scen"], cfg["drv_slot"])
    feat[:] = -7.0
    assert lib.sg_route_observation_observers(h, 0, 0.0, feat.ctypes.data, None, 0) == 0 and (feat == -7.0).all()  # no observers: nothing is written
    assert lib.sg_route_observation_observers(h, 0, 0.0, None, None, 0) == 0
    eng.set_observers(cfg["obs_scen"], cfg["obs_slot"])
    assert call() == 0
    answers = lambda: eng.route_observation(4, 2.0, observers=True)  # noqa: E731
    want = route_reference(oracle, eng.state(raw=True), scs, cfg["obs_scen"], cfg["obs_slot"], cfg["routes"], 4, 2.0)
    assert same(answers(), want)
    # every refusal, each leaving the previous routes in place
    assert call(n_=-1) == INVALID
    for name in ("scenario", "slot", "pt_off", "pts"):
        assert call(null=(name,)) == INVALID, name
    for bad_scen, bad_slot in ((-1, 0), (4, 0), (0, -1), (0, 65)):
        s2, k2 = scen.copy(), slot.copy()
        s2[3], k2[3] = bad_scen, bad_slot
        assert call(scen=s2, slot=k2) == INVALID, (bad_scen, bad_slot)
    s2, k2 = scen.copy(), slot.copy()
    s2[-1], k2[-1] = s2[0], k2[0]
    assert call(scen=s2, slot=k2) == INVALID  # a pair listed twice
    off = arrays(paths)[0]
    assert call(pt_off=off + 1) == INVALID
    swapped = off.copy()
    swapped[[4, 5]] = swapped[[5, 4]]
    assert swapped[5] < swapped[4] and call(pt_off=swapped) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        p2 = [p.copy() for p in paths]
        p2[-1][1, 0] = bad
        assert call(paths=p2) == INVALID, bad
    p2 = [p.copy() for p in paths]
    long_one = [j for j, p in enumerate(p2) if len(p) == 3][0]
    p2[long_one][0], p2[long_one][1] = (-1.5e308, 0.0), (1.5e308, 0.0)  # finite points, a length that is not
    assert call(paths=p2) == INVALID
    huge = np.array([0, 2 ** 31 + 1], np.int64)  # 2^31 segments: refused on the offsets alone, no point is read
    one = np.zeros((2, 2))
    assert lib.sg_set_routes(h, 1, scen[:1].ctypes.data, slot[:1].ctypes.data, huge.ctypes.data, one.ctypes.data) == INVALID
    assert same(answers(), want)
    for n_ahead, spacing in ((-1, 1.0), (MAX_AHEAD + 1, 1.0), (2, -1e-300), (2, np.nan), (2, np.inf)):
        assert lib.sg_route_observation(h, n_ahead, spacing, feat.ctypes.data, None, 0) == INVALID, (n_ahead, spacing)
        assert lib.sg_route_observation_observers(h, n_ahead, spacing, feat.ctypes.data, None, 0) == INVALID, (n_ahead, spacing)
    assert lib.sg_route_observation(h, 0, 0.0, None, None, 0) == INVALID and lib.sg_route_observation_observers(h, 0, 0.0, None, None, 0) == INVALID
    assert same(answers(), want)
    # the routes survive sg_reset, sg_set_observers, sg_set_drivers, a driver policy and the steps
    eng.step_drivers(cfg["actions"][:2], 2)
    eng.reset()
    eng.set_observers(cfg["obs_scen"][::-1].copy(), cfg["obs_slot"][::-1].copy())
    assert same(answers(), (want[0][::-1], want[1][::-1]))
    eng.set_observers(cfg["obs_scen"], cfg["obs_slot"])
    eng.set_drivers(cfg["drv_scen"][:3], cfg["drv_slot"][:3])
    eng.set_driver_policy([1], np.array([PS.params()]), [np.array([(0.0, 0.0), (5.0, 0.0)])])
    eng.set_drivers(cfg["drv_scen"], cfg["drv_slot"])
    assert same(answers(), want)
    # replaced by a shorter list; cleared by n == 0; forgotten by sg_upload
    fewer = {k: v for k, v in list(cfg["routes"].items())[:4]}
    eng.set_routes(*RS.route_lists(fewer))
    assert same(answers(), route_reference(oracle, eng.state(raw=True), scs, cfg["obs_scen"], cfg["obs_slot"], fewer, 4, 2.0))
    assert lib.sg_set_routes(h, 0, None, None, None, None) == 0
    none = route_reference(oracle, eng.state(raw=True), scs, cfg["obs_scen"], cfg["obs_slot"], {}, 4, 2.0)
    assert same(answers(), none) and (none[1][:, 0] == -1).all()
    assert call() == 0 and same(answers(), want)
    eng.upload(packed)
    eng.set_observers(cfg["obs_scen"], cfg["obs_slot"])
    assert same(answers(), none)
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 3. Python layers
@gpu
def test_vector_env_driver_progress(sga, oracle):
    """VectorScenarioEnv(drivers=..., driver_progress=1.0) on the column scene, one episode cut short so that it restarts within the
    run: driver_route against the yardstick on the stepped state, driver_progress the difference of consecutive arclengths,
    driver_reward the old reward plus it; the same environment without driver_progress reports what it reports today."""
    cfg = PS.column(2)
    cfg["scs"][0] = PS.cut_at(cfg["scs"][0], 1.25)
    scs = cfg["scs"]
    objs = _scenario_objects(scs)
    drivers = [[1, 2, 3, 4], [1, 2, 3, 4]]
    kw = dict(timestep=PS.DT, n=8, terminal_conditions=["max_length"], max_steer=0.7, max_accel=5.0, drivers=drivers)
    with pytest.raises(ValueError):
        sga.VectorScenarioEnv(objs, timestep=PS.DT, n=8, terminal_conditions=["max_length"], driver_progress=1.0)
    env, plain = sga.VectorScenarioEnv(objs, driver_progress=1.0, **kw), sga.VectorScenarioEnv(objs, **kw)
    assert np.array_equal(env.reset(), plain.reset())
    scen, slot = np.repeat(np.arange(2, dtype=np.int32), 4), np.tile(np.arange(1, 5, dtype=np.int32), 2)
    routes = {(int(r), int(k)): objs[r].entities[k].trajectory.data[:, 1:3] for r, k in zip(scen, slot)}
    acts = PS.caller_actions(8, [], seed=11)
    prev, prev_ok = np.zeros(8), np.zeros(8, bool)
    restarted, gained = np.zeros(2, bool), 0.0
    for k in range(30):
        obs, reward, done, info = env.step(acts[k])
        obs_p, reward_p, done_p, info_p = plain.step(acts[k])
        assert set(info_p) == {"terminal_flags", "driver_flags", "driver_info", "driver_feat", "driver_reward", "driver_done"}
        assert set(info) == set(info_p) | {"driver_route", "driver_progress"}
        assert np.array_equal(obs, obs_p) and np.array_equal(reward, reward_p) and np.array_equal(done, done_p)
        for key in info_p:
            if key != "driver_reward":
                assert np.array_equal(info[key], info_p[key]), (k, key)
        assert np.array_equal(info_p["driver_reward"], np.where((info_p["driver_flags"] & 6) != 0, -1.0, 0.01))
        if not done.any():  # (an auto-reset has replaced the stepped state otherwise)
            want = route_reference(oracle, env.engine.state(raw=True), scs, scen, slot, routes, 0, 0.0)
            assert np.array_equal(_bits(info["driver_route"]), _bits(want[0])), k
        s0 = info["driver_route"][:, 8]
        on = (info["driver_flags"] & 1) != 0
        want_progress = np.where(on & prev_ok, s0 - prev, 0.0)
        assert np.array_equal(_bits(info["driver_progress"]), _bits(want_progress)), k
        assert np.array_equal(_bits(info["driver_reward"]), _bits(info_p["driver_reward"] + 1.0 * want_progress)), k
        gained += float(want_progress.sum())
        prev, prev_ok = s0.copy(), on & ~done[scen]
        restarted |= done
    assert restarted[0] and not restarted[1] and gained > 20.0  # (the drivers drove, along their routes)
    env.close()
    plain.close()


@gpu
def test_state_route_observation_and_torch_forms(sga, oracle):
    """State.route_observation through ScenarioGym (routes default to every entity's own recording; ScenarioGym.set_routes replaces
    them), and VectorScenarioEnv.route_observation / observe_entities_routes in their numpy and torch forms."""
    cfg = PS.column(2)
    scs = cfg["scs"]
    objs = _scenario_objects(scs)
    E = PS.COLUMN_E
    gym = sga.ScenarioGym(timestep=PS.DT, terminal_conditions=[])
    gym.set_scenario(objs[0])
    ents = gym.state.scenario.entities
    ego = scs[0]["ego"]
    routes = {(0, k): np.asarray(e.trajectory.data, F)[:, 1:3] for k, e in enumerate(ents)}
    for k in range(3):
        gym.step()
        st = gym._b.engine.state(raw=True)
        feat, info = route_reference(oracle, st, scs[:1], np.zeros(E, int), np.arange(E), routes, 4, 2.0)
        for j in (ego, 1, 7):
            o = gym.state.route_observation(4, 2.0, entity=None if j == ego else ents[j])
            assert isinstance(o, sga.RouteObservation) and o.entity is ents[j] and o.present == bool(st["present"][0, j])
            assert np.array_equal(_bits(o.features), _bits(feat[j])) and (o.segment, o.recording) == tuple(info[j])
            assert (o.log_divergence, o.progress, o.remaining) == (feat[j, 2], feat[j, 8], feat[j, 9])
    other = {(0, 1): PS.PATH}
    gym._b.set_routes([{1: PS.PATH}])
    st = gym._b.engine.state(raw=True)
    feat, info = route_reference(oracle, st, scs[:1], [0, 0], [1, 2], other, 2, 1.0)
    o1, o2 = gym.state.route_observation(2, 1.0, entity=ents[1]), gym.state.route_observation(2, 1.0, entity=ents[2])
    assert np.array_equal(_bits(o1.features), _bits(feat[0])) and o1.segment == info[0, 0] >= 0
    assert np.array_equal(_bits(o2.features), _bits(feat[1])) and o2.segment == -1
    gym.close()
    drivers = [[1, 2], [3]]
    scen, slot = np.array([0, 0, 1], np.int32), np.array([1, 2, 3], np.int32)
    egos = np.array([sc["ego"] for sc in scs], np.int32)
    rec = {(int(r), int(k)): np.asarray(objs[r].entities[k].trajectory.data, F)[:, 1:3] for r, k in zip(scen, slot)}
    for torch_obs in (False, True):
        env = sga.VectorScenarioEnv(objs, timestep=PS.DT, n=8, terminal_conditions=["max_length"], max_steer=0.7, max_accel=5.0, drivers=drivers,
                                    torch_obs=torch_obs)
        env.reset()
        env.step(np.array([[1.0, 0.1], [0.5, -0.1], [2.0, 0.05]]))
        seen, own = env.observe_entities_routes(3, 1.5), env.route_observation(3, 1.5)
        if torch_obs:
            assert all(t.is_cuda for t in seen) and all(t.is_cuda for t in own)
            seen, own = [t.cpu().numpy() for t in seen], [t.cpu().numpy() for t in own]
        st = env.engine.state(raw=True)
        assert list(seen[2]) == list(scen) and list(seen[3]) == list(slot)
        assert same(seen[:2], route_reference(oracle, st, scs, scen, slot, rec, 3, 1.5))
        assert same(own, route_reference(oracle, st, scs, np.arange(2), egos, rec, 3, 1.5)) and (own[1][:, 0] == -1).all()
        env.set_routes([{int(egos[0]): PS.PATH}, {}])
        own = env.route_observation(3, 1.5)
        own = [t.cpu().numpy() for t in own] if torch_obs else own
        assert same(own, route_reference(oracle, st, scs, np.arange(2), egos, {(0, int(egos[0])): PS.PATH}, 3, 1.5)) and own[1][0, 0] >= 0
        env.close()
