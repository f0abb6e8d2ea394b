"""The built-in driver policy: sg_set_driver_policy / sg_driver_policy_actions / sg_step_drivers_policy (driver_policy_kernel) and the
Python layers over them.

The yardstick is policy_reference: the definition in include/sgym.h at sg_set_driver_policy restated in scalar fp64, every sine and
cosine from oracle.sincos.  The device must equal it bit for bit.

CPU  the scenes of policy_scenes.py held to their purpose: a plain closed loop on the column scene; every case the open-loop scenes name
GPU  1. open loop at E = 3, 64, 65, 520, host and device outputs
     2. closed loop three ways on the column and the mixed scene
     3. lifecycle and refusals
     4. VectorScenarioEnv(drivers=..., traffic=...)
"""
import ctypes as C

import numpy as np
import pytest

import policy_scenes as PS
from box_scenes import quads_meet_exact
from test_drivers import _assert_same, _bits, _scenario_objects, _snapshot

gpu = pytest.mark.gpu
INF = float("inf")
F = np.float64


@pytest.fixture(scope="module")
def sga():
    import scenario_gym_amd as sga

    return sga


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def segment_rows(path):
    """The rows sg_set_lanes builds for one polyline: (ax, ay, ex, ey, L2, len, cum, bx, by) per segment, and total."""
    rows, cum = [], F(0.0)
    for a, b in zip(path[:-1], path[1:]):
        ax, ay, bx, by = F(a[0]), F(a[1]), F(b[0]), F(b[1])
        ex, ey = bx - ax, by - ay
        L2 = ex * ex + ey * ey
        ln = np.sqrt(L2)
        rows.append((ax, ay, ex, ey, L2, ln, cum, bx, by))
        cum = cum + ln
    return rows, (rows[-1][6] + rows[-1][5] if rows else F(0.0))


def lane_project(g, px, py):
    """The point-to-segment rule of sg_lane_observation: (d2, dx, dy, t)."""
    ax, ay, ex, ey, L2, _, _, bx, by = g
    wx, wy = px - ax, py - ay
    t = (wx * ex + wy * ey) / L2
    if L2 == 0.0 or not (t > 0.0):
        t, cx, cy = F(0.0), ax, ay
    elif t >= 1.0:
        t, cx, cy = F(1.0), bx, by
    else:
        cx, cy = ax + t * ex, ay + t * ey
    dx, dy = px - cx, py - cy
    return dx * dx + dy * dy, dx, dy, t


def policy_one(oracle, poses, vels, present, speed, bbox, so, prm, path):
    """One policy driver, slot so of a scenario given as poses / vels [E, 6], present [E], speed [E] (the SG_F_CTRL + 0 cells), bbox
    [E, 4].  Returns (actions [2], info [2], feat [6], extra): extra holds the intermediate values the scene tests ask about."""
    P = PS
    if not present[so]:
        return [0.0, 0.0], [-1, -1], [0.0] * 6, dict(absent=True)
    x, y, v = F(poses[so, 0]), F(poses[so, 1]), F(speed[so])
    s, c = (F(q) for q in oracle.sincos(poses[so, 3]))
    Wo, Lo, cxo, cyo = (F(q) for q in bbox[so])
    front = cxo + F(0.5) * Lo
    ex = dict(absent=False, v=v)
    # the path term
    rows, total = segment_rows(path)
    d2s = [lane_project(g, x, y)[0] for g in rows]
    best = -1
    for i, d2 in enumerate(d2s):
        if np.isfinite(d2) and (best < 0 or d2 < d2s[best]):
            best = i
    steer, off, se, s0, rem = F(0.0), F(0.0), F(0.0), F(0.0), F(INF)
    ex.update(d2=d2s, best=best, lens=[g[5] for g in rows])
    if best >= 0:
        g = rows[best]
        _, dx, dy, t = lane_project(g, x, y)
        ln = g[5]
        ux, uy = (g[2] / ln, g[3] / ln) if ln != 0.0 else (F(0.0), F(0.0))
        off = ux * dy - uy * dx
        se, ce = s * ux - c * uy, c * ux + s * uy
        ex["ce"] = ce
        if ce < 0.0:
            se = F(1.0) if se >= 0.0 else F(-1.0)
        s0 = g[6] + t * ln
        rem = total - s0
        steer = -(prm[P.K_PSI] * se + (prm[P.K_E] * off) / (prm[P.K_SOFT] + abs(v)))
    # the lead
    left, right = (cyo + F(0.5) * Wo) + prm[P.HALF], (cyo - F(0.5) * Wo) - prm[P.HALF]
    lead, gap, others = -1, F(INF), {}
    for e in range(len(present)):
        if e == so:
            continue
        sn, cn = (F(q) for q in oracle.sincos(poses[e, 3]))
        We, Le, cxe, cye = (F(q) for q in bbox[e])
        qx, qy = F(poses[e, 0]) + (cxe * cn - cye * sn), F(poses[e, 1]) + (cxe * sn + cye * cn)
        dx, dy = qx - x, qy - y
        lon, lat = dx * c + dy * s, dy * c - dx * s
        cr, sr = cn * c + sn * s, sn * c - cn * s
        hl, hw = F(0.5) * (abs(Le * cr) + abs(We * sr)), F(0.5) * (abs(Le * sr) + abs(We * cr))
        g = (lon - hl) - front
        conds = (bool(lat - hw <= left), bool(lat + hw >= right), bool(lon + hl > front), bool(g <= prm[P.REACH]))
        others[e] = dict(present=bool(present[e]), conds=conds, gap=g, cr=cr, edge=(lat - hw, lat + hw), candidate=bool(present[e]) and all(conds))
        if others[e]["candidate"] and (lead < 0 or g < gap):  # (ascending slots: the lower slot keeps a tie)
            lead, gap = e, g
    dv = v - (F(vels[lead, 0]) * c + F(vels[lead, 1]) * s) if lead >= 0 else F(0.0)
    ex.update(others=others, left=left, right=right)
    # the acceleration
    A_, vr = prm[P.A], v / prm[P.V0]
    free = F(1.0) - (vr * vr) * (vr * vr)
    root = F(2.0) * np.sqrt(A_ * prm[P.B])

    def idm(g, d):
        q = v * prm[P.T] + (v * d) / root
        ss = prm[P.S0] + (q if q > 0.0 else F(0.0))
        gg = g if g > prm[P.GAP_MIN] else prm[P.GAP_MIN]
        rr = ss / gg
        return A_ * (free - rr * rr)

    acc = idm(gap, dv) if lead >= 0 else A_ * free
    ex["ae_binds"] = False
    if best >= 0:
        ae = idm(rem, v)
        ex["ae_binds"] = bool(ae < acc)
        acc = ae if ae < acc else acc
    return [acc, steer], [lead, best], [gap, dv, off, se, s0, rem], ex


def policy_reference(oracle, st, bbox, scen, slot, params, paths):
    """The definition for the policy drivers (scen[j], slot[j]) on a batch state as RolloutEngine.state(raw=True) gives it (poses, vels,
    present, ctrl_state); bbox [R, E, 4].  Returns (actions [m, 2], info [m, 2] int32, feat [m, 6], extras)."""
    m = len(scen)
    actions, info, feat, extras = np.zeros((m, 2)), np.zeros((m, 2), np.int32), np.zeros((m, 6)), []
    with np.errstate(all="ignore"):
        for j in range(m):
            r = int(scen[j])
            a, i, f, ex = policy_one(oracle, st["poses"][r], st["vels"][r], st["present"][r], st["ctrl_state"][r][:, 0], bbox[r], int(slot[j]),
                                     np.asarray(params[j], F), np.asarray(paths[j], F).reshape(-1, 2))
            actions[j], info[j], feat[j] = a, i, f
            extras.append(ex)
    return actions, info, feat, extras


def same(got, want):
    """actions and feat bit for bit, info exactly."""
    return (np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(np.asarray(got[1]), want[1]) and
            np.array_equal(_bits(got[2]), _bits(want[2])))


def _bbox_of(scs):
    return np.array([s["bbox"] for s in scs])


def nominal_state(cfg):
    """The state the open-loop scenes are written for, by hand: every entity at its first knot, in the scene iff its recording has
    started; the policy drivers at their nominal speed."""
    scs = cfg["scs"]
    R, E = len(scs), len(scs[0]["etype"])
    poses, present, speed = np.zeros((R, E, 6)), np.zeros((R, E), bool), np.zeros((R, E))
    for r, sc in enumerate(scs):
        first = sc["knots"][sc["knot_off"][:-1]]
        poses[r], present[r] = first[:, 1:], first[:, 0] <= 0.0
    pr, pk = cfg["scen"][cfg["driver"]], cfg["slot"][cfg["driver"]]
    speed[pr, pk] = cfg["nominal_v"]
    vels = np.zeros((R, E, 6))
    return dict(poses=poses, vels=vels, present=present, ctrl_state=speed[..., None] * np.array([1.0, 0, 0, 0]))


# ---------------------------------------------------------------------------------------------------------------- CPU: the scenes
@pytest.mark.parametrize("E", [3, 64, 65, 520])
def test_open_loop_scenes_hold_every_case(oracle, E):
    """Every case the open-loop comparison is meant to cover is in the scenes, judged by the yardstick's own intermediate values."""
    cfg = PS.open_loop(E)
    scen, slot = cfg["scen"][cfg["driver"]], cfg["slot"][cfg["driver"]]
    assert (np.diff(cfg["driver"]) > 0).all() and not np.array_equal(cfg["driver"], np.arange(len(scen)))  # (a caller-run driver comes first)
    act, info, feat, extras = policy_reference(oracle, nominal_state(cfg), _bbox_of(cfg["scs"]), scen, slot, cfg["params"], cfg["paths"])
    by = {role: j for j, (_, role) in enumerate(cfg["who"])}
    X = lambda role: PS.slots_of(E, cfg["who"][by[role]][0])[1]  # noqa: E731
    Y = lambda role: PS.slots_of(E, cfg["who"][by[role]][0])[2]  # noqa: E731
    assert sorted(len(p) for p in cfg["paths"])[:3] == [0, 1, 2] and {65, 130} <= {len(p) for p in cfg["paths"]}
    # zero-length segments in the middle and at the end of a path, a pose equidistant from two segments (the lower index wins)
    ex = extras[by["equidistant"]]
    assert ex["lens"][1] == 0.0 and ex["lens"][3] == 0.0 and ex["lens"][0] > 0.0 and ex["lens"][2] > 0.0
    assert ex["d2"][0] == ex["d2"][2] == min(ex["d2"]) and info[by["equidistant"], 1] == 0
    ex = extras[by["zero_first"]]
    assert ex["lens"][0] == 0.0 and ex["d2"][0] == ex["d2"][1] and info[by["zero_first"], 1] == 0
    # facing against the path; off-axis box centres, a lead rotated by 90 degrees, in another block than the driver
    j = by["against"]
    sc = cfg["scs"][cfg["who"][j][0]]
    assert extras[j]["ce"] < 0.0 and abs(feat[j, 3]) == 1.0 and info[j, 0] == Y("against")
    assert sc["bbox"][slot[j], 3] != 0.0 and sc["bbox"][Y("against"), 3] != 0.0 and abs(extras[j]["others"][Y("against")]["cr"]) < 1e-12
    assert E < 65 or Y("against") // 64 != slot[j] // 64
    # two candidates with bit-equal gap: the lower slot
    j = by["tie"]
    o = extras[j]["others"]
    assert o[X("tie")]["candidate"] and o[Y("tie")]["candidate"] and _bits(np.array([o[X("tie")]["gap"]]))[0] == _bits(np.array([o[Y("tie")]["gap"]]))[0]
    assert info[j, 0] == min(X("tie"), Y("tie")) and feat[j, 0] == 16.0
    # beside the driver with a negative gap; an absent entity inside the corridor, nearer still
    j = by["beside"]
    o = extras[j]["others"]
    assert info[j, 0] == X("beside") and feat[j, 0] == -3.0 and info[j, 1] == -1 and feat[j, 5] == INF
    assert not o[Y("beside")]["present"] and all(o[Y("beside")]["conds"]) and o[Y("beside")]["gap"] < feat[j, 0]
    # exactly at REACH and one ulp beyond it; one ulp of its own coordinate outside the corridor on either side, nearer than the lead
    j, k = by["reach"], by["beyond"]
    assert info[j, 0] == X("reach") and feat[j, 0] == cfg["params"][j][PS.REACH] == 16.0
    o = extras[k]["others"][X("beyond")]
    assert info[k, 0] == -1 and o["conds"] == (True, True, True, False) and o["gap"] == np.nextafter(16.0, 17.0)
    o = extras[j]["others"][Y("reach")]
    assert o["conds"] == (False, True, True, True) and 0.0 < o["edge"][0] - extras[j]["left"] <= 2.0 ** -51 and o["gap"] < 16.0
    o = extras[k]["others"][Y("beyond")]
    assert o["conds"] == (True, False, True, True) and 0.0 < extras[k]["right"] - o["edge"][1] <= 2.0 ** -51
    # a driver that has not spawned; REACH = +inf
    assert extras[by["unspawned"]]["absent"] and not act[by["unspawned"]].any() and (info[by["unspawned"]] == -1).all()
    assert cfg["params"][by["far"]][PS.REACH] == INF and info[by["far"], 0] == Y("far") and 400.0 < feat[by["far"], 0] < INF
    # a negative speed
    assert extras[by["reverse"]]["v"] < 0.0 and info[by["reverse"], 0] == X("reverse")
    assert np.isfinite(act).all()


def _interp(knots, t):
    """The recorded pose at time t (linear between knots), None outside the recording."""
    if t < knots[0, 0] or t > knots[-1, 0]:
        return None
    i = min(max(int(np.searchsorted(knots[:, 0], t, "right")) - 1, 0), len(knots) - 2)
    u = (t - knots[i, 0]) / (knots[i + 1, 0] - knots[i, 0])
    return knots[i, 1:] + u * (knots[i + 1, 1:] - knots[i, 1:])


def numpy_closed_loop(oracle, cfg, steps, caller=None):
    """The policy and VehicleController._step in plain numpy on the scenes of cfg: per step the boxes' corners, the followers'
    speeds, whether each has a lead, whether its path-end term binds.  Returns dict(min_sep, speeds [steps + 1, m], lead [steps, m],
    ae [steps, m], overlap)."""
    scs = cfg["scs"]
    R, E = len(scs), len(scs[0]["etype"])
    bbox = _bbox_of(scs)
    knots = [[sc["knots"][sc["knot_off"][e]:sc["knot_off"][e + 1]] for e in range(E)] for sc in scs]
    poses, vels, present, speed = np.zeros((R, E, 6)), np.zeros((R, E, 6)), np.zeros((R, E), bool), np.zeros((R, E))
    for r in range(R):
        for e in range(E):
            p = _interp(knots[r][e], 0.0)
            present[r, e] = p is not None
            if p is not None:
                k = knots[r][e]
                poses[r, e] = p
                vels[r, e] = (k[1, 1:] - k[0, 1:]) / (k[1, 0] - k[0, 0])
                speed[r, e] = np.hypot(vels[r, e, 0], vels[r, e, 1])
    pr, pk = cfg["scen"][cfg["driver"]], cfg["slot"][cfg["driver"]]
    is_driver = np.zeros((R, E), bool)
    is_driver[cfg["scen"], cfg["slot"]] = True
    out = dict(speeds=[speed[pr, pk].copy()], lead=[], ae=[], gap=[], overlap=False)
    t = 0.0
    for k in range(steps):
        st = dict(poses=poses, vels=vels, present=present, ctrl_state=speed[..., None] * np.array([1.0, 0, 0, 0]))
        act, info, feat, extras = policy_reference(oracle, st, bbox, pr, pk, cfg["params"], cfg["paths"])
        out["lead"].append(info[:, 0] >= 0)
        out["ae"].append([ex["ae_binds"] for ex in extras])
        out["gap"].append(feat[:, 0])
        merged = np.zeros((len(cfg["scen"]), 2)) if caller is None else caller[k].copy()
        merged[cfg["driver"]] = act
        next_t = t + PS.DT
        dt = next_t - t
        new = poses.copy()
        for d, (r, e) in enumerate(zip(cfg["scen"], cfg["slot"])):  # VehicleController._step
            ms, ma = scs[r]["ctrl"][e, 0], scs[r]["ctrl"][e, 1]
            a, s = min(max(merged[d, 0], -ma), ma), min(max(merged[d, 1], -ms), ms)
            h = poses[r, e, 3]
            new[r, e, 0] += speed[r, e] * np.cos(h) * dt
            new[r, e, 1] += speed[r, e] * np.sin(h) * dt
            new[r, e, 3] += speed[r, e] * np.tan(s) / bbox[r, e, 1] * dt
            speed[r, e] = max(0.0, speed[r, e] + a * dt)
        for r in range(R):
            for e in range(E):
                if not is_driver[r, e]:
                    p = _interp(knots[r][e], next_t)
                    present[r, e] = p is not None
                    if p is not None:
                        new[r, e] = p
        vels = (new - poses) / dt
        poses, t = new, next_t
        out["speeds"].append(speed[pr, pk].copy())
        for r in range(R):
            idx = [e for e in range(E) if present[r, e] and abs(poses[r, e, 1]) < 500.0]  # (the fillers stand a kilometre away)
            cor = {e: oracle.corners(poses[r, e], bbox[r, e]) for e in idx}
            for i in idx:
                for j in idx:
                    if i < j and quads_meet_exact(cor[i], cor[j]):
                        out["overlap"] = True
    for key in ("speeds", "lead", "ae", "gap"):
        out[key] = np.array(out[key])
    return out


def test_column_scene_does_what_it_is_for(oracle):
    """The column scene in a plain numpy closed loop (policy_reference and a five-line VehicleController._step), 60 steps at dt = 0.1:
    no two boxes ever overlap (the exact test of box_scenes.py); every follower ends within SPEED_MARGIN = 0.5 m/s of the lead's
    4 m/s; every follower has a lead in some step; some driver's path-end term binds in some step.
    Conditions on the scene, not measurements of the device.  Observed: the smallest gap of the run 7.8 m; the worst final speed
    error 0.18 m/s (margin 0.5); every follower has a lead in all 60 steps; the first follower of either scenario has the path-end
    term binding in its last 4 steps."""
    cfg = PS.column()
    out = numpy_closed_loop(oracle, cfg, PS.STEPS)
    worst = np.abs(out["speeds"][-1] - PS.LEAD_SPEED).max()
    print("column: worst final speed error", worst, "smallest gap", out["gap"].min(), "lead steps", out["lead"].sum(0), "ae steps", out["ae"].sum(0))
    assert not out["overlap"] and out["gap"].min() > 0.0
    assert worst <= PS.SPEED_MARGIN
    assert out["lead"].any(axis=0).all()
    assert out["ae"].any()


# ------------------------------------------------------------------------------------------------------------------------ GPU
TERMS = ["max_length"]


def _engine(sga, cfg, **kw):
    scs = cfg["scs"]
    eng = sga.RolloutEngine(len(scs), len(scs[0]["etype"]), timestep=PS.DT, terminal_conditions=TERMS, event_capacity=16, **kw)
    eng.upload(PS.pack(scs))
    eng.set_drivers(cfg["scen"], cfg["slot"])
    return eng


def _set_policy(eng, cfg):
    eng.set_driver_policy(cfg["driver"], cfg["params"], cfg["paths"])


def _want(oracle, eng, cfg):
    return policy_reference(oracle, eng.state(raw=True), _bbox_of(cfg["scs"]), cfg["scen"][cfg["driver"]], cfg["slot"][cfg["driver"]],
                            cfg["params"], cfg["paths"])


# ---------------------------------------------------------------------------------------------------------------- 1. open loop
@gpu
@pytest.mark.parametrize("E", [3, 64, 65, 520])
def test_open_loop_against_the_yardstick(sga, oracle, E):
    """sg_driver_policy_actions on the reset state (the poses exactly as the scenes write them) and after PRE steps of
    sg_step_drivers (one driver reversing by then), host outputs and device outputs, with and without the optional arrays."""
    import torch

    cfg = PS.open_loop(E)
    eng = _engine(sga, cfg)
    _set_policy(eng, cfg)
    m = len(cfg["driver"])
    nominal = policy_reference(oracle, nominal_state(cfg), _bbox_of(cfg["scs"]), cfg["scen"][cfg["driver"]], cfg["slot"][cfg["driver"]],
                               cfg["params"], cfg["paths"])
    rev = [j for j, (_, role) in enumerate(cfg["who"]) if role == "reverse"][0]
    for stage in ("reset", "stepped"):
        if stage == "stepped":
            eng.step_drivers(cfg["pre_actions"], PS.PRE)
        want = _want(oracle, eng, cfg)
        got = eng.driver_policy_actions()
        assert same(got, want), stage
        dev = eng.driver_policy_actions(torch_out=True)
        assert same([t.cpu().numpy() for t in dev], want), stage
        # the optional arrays left out: the actions alone, and guard words behind them untouched
        buf = np.full(2 * m + 4, -7.0)
        assert eng.lib.sg_driver_policy_actions(eng.h, buf.ctypes.data, None, None, 0) == 0
        assert np.array_equal(_bits(buf[:2 * m].reshape(m, 2)), _bits(want[0])) and (buf[2 * m:] == -7.0).all()
        t = torch.full((2 * m + 4,), -7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        assert eng.lib.sg_driver_policy_actions(eng.h, t.data_ptr(), None, None, 1) == 0
        eng.synchronize()
        assert np.array_equal(_bits(t.cpu().numpy()[:2 * m].reshape(m, 2)), _bits(want[0])) and (t.cpu().numpy()[2 * m:] == -7.0).all()
        if stage == "reset":  # the device's reset state is the hand-made one as far as the policy reads it (all but the reverser's speed)
            keep = np.arange(m) != rev
            assert np.array_equal(got[1][keep], nominal[1][keep]) and np.array_equal(_bits(got[2][keep]), _bits(nominal[2][keep]))
        else:
            assert want[3][rev]["v"] < 0.0 and want[1][rev, 0] >= 0
    eng.close()


# -------------------------------------------------------------------------------------------------------------- 2. closed loop
N_CLOSED = 40


def _closed_cfg(name):
    return PS.column(2, mixed=(name == "mixed"))


@gpu
@pytest.mark.parametrize("name", ["column", "mixed"])
def test_closed_loop_three_ways(sga, oracle, name):
    """(a) one sg_step_drivers_policy call of 40 steps, (b) forty calls of one step, (c) forty rounds of sg_driver_policy_actions, a
    host merge and sg_step_drivers: the whole readable state bit for bit; the caller's device actions untouched; on (b) every step's
    actions against the yardstick; the conditions of the column scene on the device run, through sg_entity_status_observers."""
    import torch

    cfg = _closed_cfg(name)
    nd = len(cfg["scen"])
    acts = PS.caller_actions(nd, cfg["driver"], seed=3)[:N_CLOSED]
    d_acts = torch.as_tensor(acts, device="cuda:0").contiguous()
    keep = d_acts.clone()
    a, b, c = (_engine(sga, cfg) for _ in range(3))
    for e_ in (a, b, c):
        _set_policy(e_, cfg)
    _assert_same(_snapshot(a), _snapshot(b), "reset")
    a.step_drivers_policy(d_acts, N_CLOSED)
    assert torch.equal(d_acts, keep)
    fr, fk = np.array([r for r, _ in cfg["follow"]], np.int32), np.array([k for _, k in cfg["follow"]], np.int32)
    R = len(cfg["scs"])
    b.set_observers(np.concatenate([fr, np.arange(R, dtype=np.int32)]), np.concatenate([fk, np.full(R, cfg["lead_slot"], np.int32)]))
    had_lead, collided, speeds = np.zeros(len(fr), bool), False, None
    for k in range(N_CLOSED):
        want = _want(oracle, b, cfg)
        got = b.driver_policy_actions()
        assert same(got, want), k
        had_lead |= want[1][:, 0] >= 0
        b.step_drivers_policy(d_acts[k:k + 1].contiguous(), 1)
        merged = acts[k].copy()
        merged[cfg["driver"]] = c.driver_policy_actions()[0]
        c.step_drivers(merged[None], 1)
        flags, _, feat = b.entity_status_observers()
        collided |= bool((flags & 2).any())
        speeds = feat[:, 0]
    assert torch.equal(d_acts, keep)
    one = _snapshot(a)
    _assert_same(one, _snapshot(b), "one call against forty")
    _assert_same(one, _snapshot(c), "one call against the loop of sg_driver_policy_actions and sg_step_drivers")
    # the scene's conditions on the device run (40 of the 60 steps: the followers are on their way to the lead's speed)
    assert not collided and had_lead.all()
    assert (np.abs(speeds[:len(fr)] - speeds[len(fr):][fr]) <= PS.SPEED_MARGIN).all()
    # and after the resets the closed loop repeats bit for bit
    a.reset()
    a.step_drivers_policy(d_acts, N_CLOSED)
    _assert_same(one, _snapshot(a), "after sg_reset")
    for e_ in (a, b, c):
        e_.close()
    # (the path's end binds in the last steps of the 60, beyond these 40: test_closed_loop_reaches_the_path_end)


@gpu
def test_closed_loop_reaches_the_path_end(sga, oracle):
    """The column scene for its 60 steps in one call: at the end some follower's path-end term binds, every follower is within
    SPEED_MARGIN of the lead's speed and has a lead, and nobody has collided."""
    cfg = PS.column(2)
    eng = _engine(sga, cfg)
    _set_policy(eng, cfg)
    fr, fk = np.array([r for r, _ in cfg["follow"]], np.int32), np.array([k for _, k in cfg["follow"]], np.int32)
    R = len(cfg["scs"])
    eng.set_observers(np.concatenate([fr, np.arange(R, dtype=np.int32)]), np.concatenate([fk, np.full(R, cfg["lead_slot"], np.int32)]))
    eng.step_drivers_policy(None, PS.STEPS - 1)
    want = _want(oracle, eng, cfg)
    assert same(eng.driver_policy_actions(), want)
    assert any(ex["ae_binds"] for ex in want[3]) and (want[1][:, 0] >= 0).all()
    eng.step_drivers_policy(None, 1)
    flags, _, feat = eng.entity_status_observers()
    assert not (flags & 2).any() and (np.abs(feat[:len(fr), 0] - feat[len(fr):, 0][fr]) <= PS.SPEED_MARGIN).all()
    rows, _ = eng.metrics()
    assert (rows["n_collisions"] == 0).all()
    eng.close()


# ------------------------------------------------------------------------------------------------------ 3. lifecycle and refusals
def _pol(driver, params, paths, pt_off=None):
    """(sg_driver_policy, the arrays it points into)."""
    import scenario_gym_amd._lib as L

    driver = np.ascontiguousarray(driver, np.int64)
    params = np.ascontiguousarray(params, np.float64)
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64) if pt_off is None else np.ascontiguousarray(pt_off, np.int64)
    pts = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in paths]) if paths else np.zeros((0, 2)))
    return L.SgDriverPolicy(len(driver), driver.ctypes.data, params.ctypes.data, off.ctypes.data, pts.ctypes.data), (driver, params, off, pts)


@gpu
def test_lifecycle_and_refusals(sga, oracle):
    import scenario_gym_amd._lib as L

    INVALID, STATE = -1, -3
    cfg = PS.column(2, mixed=True)
    nd, m = len(cfg["scen"]), len(cfg["driver"])
    packed = PS.pack(cfg["scs"])
    eng = sga.RolloutEngine(2, PS.COLUMN_E, timestep=PS.DT, terminal_conditions=TERMS, event_capacity=16)
    lib, h = eng.lib, eng.h
    good, keep_good = _pol(cfg["driver"], cfg["params"], cfg["paths"])
    out = np.zeros((m, 2))
    assert lib.sg_set_driver_policy(h, C.byref(good)) == STATE and lib.sg_step_drivers_policy(h, 1, None, 0) == STATE  # before sg_upload
    assert lib.sg_driver_policy_actions(h, out.ctypes.data, None, None, 0) == STATE
    eng.upload(packed)
    assert lib.sg_set_driver_policy(h, C.byref(good)) == STATE and lib.sg_step_drivers_policy(h, 1, None, 0) == STATE  # no driver list
    eng.set_drivers(cfg["scen"], cfg["slot"])
    assert lib.sg_step_drivers_policy(h, 1, None, 0) == STATE  # no policy
    out[:] = -7.0
    assert lib.sg_driver_policy_actions(h, out.ctypes.data, None, None, 0) == 0 and (out == -7.0).all()  # no policy: nothing is written
    assert lib.sg_driver_policy_actions(h, None, None, None, 0) == 0
    _set_policy(eng, cfg)
    twin = _engine(sga, cfg)
    _set_policy(twin, cfg)

    def refused(driver=cfg["driver"], params=cfg["params"], paths=cfg["paths"], pt_off=None, null=None, m_=None):
        pol, keep = _pol(driver, params, paths, pt_off)
        if null:
            setattr(pol, null, None)
        if m_ is not None:
            pol.m = m_
        return lib.sg_set_driver_policy(h, C.byref(pol)) == INVALID

    assert refused(m_=-1) and refused(null="driver") and refused(null="params") and refused(null="pt_off") and refused(null="pts")
    one = cfg["driver"].copy()
    for bad in (-1, nd):
        one[:] = cfg["driver"]
        one[0] = bad
        assert refused(driver=one)
    assert refused(driver=cfg["driver"][::-1].copy()) and refused(driver=np.full(m, cfg["driver"][0]))  # descending; not strictly ascending
    off = np.concatenate([[0], np.cumsum([len(p) for p in cfg["paths"]])])
    assert refused(pt_off=off + 1) and refused(pt_off=np.concatenate([off[:1], off[2:3], off[1:2], off[3:]]))

    def with_param(col, value):
        p = cfg["params"].copy()
        p[m - 1, col] = value
        return p

    for col in range(PS.NPARAM):
        assert refused(params=with_param(col, np.nan)), col
    for col in (PS.V0, PS.A, PS.B, PS.K_SOFT, PS.GAP_MIN):
        for value in (0.0, -1.0, np.inf):
            assert refused(params=with_param(col, value)), (col, value)
    for col in (PS.T, PS.S0, PS.HALF, PS.REACH):
        assert refused(params=with_param(col, -1e-300)), col
    for col in (PS.T, PS.S0, PS.HALF, PS.K_PSI, PS.K_E):
        assert refused(params=with_param(col, np.inf)) and refused(params=with_param(col, -np.inf)), col
    bad_path = [p.copy() for p in cfg["paths"]]
    bad_path[1][3, 1] = np.nan
    assert refused(paths=bad_path)
    assert lib.sg_step_drivers_policy(h, 0, None, 0) == INVALID and lib.sg_step_drivers_policy(h, -2, None, 0) == INVALID
    assert lib.sg_driver_policy_actions(h, None, None, None, 0) == INVALID
    # what is allowed: REACH = +inf, T = S0 = HALF = 0, negative gains -- on a third handle, whose policy is then replaced
    ok = cfg["params"].copy()
    ok[:, [PS.T, PS.S0, PS.HALF]] = 0.0
    ok[:, PS.REACH], ok[:, PS.K_PSI] = np.inf, -1.0
    third = _engine(sga, cfg)
    third.set_driver_policy(cfg["driver"], ok, cfg["paths"])
    third.step_drivers_policy(None, 2)
    third.close()
    # the refused calls left the policy in place and working: the handle goes on as its twin does
    acts = PS.caller_actions(nd, cfg["driver"], seed=5)
    eng.step_drivers_policy(acts[:5], 5)
    twin.step_drivers_policy(acts[:5], 5)
    _assert_same(_snapshot(eng), _snapshot(twin), "after the refusals")
    # sg_step_drivers on a handle with a policy equals a handle without one
    plain = _engine(sga, cfg)
    eng.reset()
    eng.step_drivers(acts[:5], 5)
    plain.step_drivers(acts[:5], 5)
    _assert_same(_snapshot(eng), _snapshot(plain), "sg_step_drivers with a policy set")
    # the resets, sg_step and sg_step_drivers kept it
    eng.reset_scenarios(np.array([1, 0], np.uint8))
    fed = np.full((2, PS.COLUMN_E, 6), np.nan)
    eng.set_external_poses(fed)
    eng.step(1)
    assert same(eng.driver_policy_actions(), _want(oracle, eng, cfg))
    eng.reset()
    twin.reset()
    eng.step_drivers_policy(acts[:5], 5)
    twin.step_drivers_policy(acts[:5], 5)
    _assert_same(_snapshot(eng), _snapshot(twin), "after the resets")
    # NULL or m == 0 clears; sg_set_drivers forgets the policy, replacing or clearing the list; so does sg_upload
    assert lib.sg_set_driver_policy(h, None) == 0 and lib.sg_step_drivers_policy(h, 1, None, 0) == STATE
    _set_policy(eng, cfg)
    empty, keep_empty = _pol(np.zeros(0, np.int64), np.zeros((0, PS.NPARAM)), [])
    assert lib.sg_set_driver_policy(h, C.byref(empty)) == 0 and lib.sg_step_drivers_policy(h, 1, None, 0) == STATE
    _set_policy(eng, cfg)
    eng.set_drivers(cfg["scen"], cfg["slot"])
    assert lib.sg_step_drivers_policy(h, 1, None, 0) == STATE and eng._n_pol == 0
    _set_policy(eng, cfg)
    eng.set_drivers([], [])
    eng.set_drivers(cfg["scen"], cfg["slot"])
    assert lib.sg_step_drivers_policy(h, 1, None, 0) == STATE
    _set_policy(eng, cfg)
    assert lib.sg_step_drivers_policy(h, 1, None, 0) == 0
    eng.upload(packed)
    eng.set_drivers(cfg["scen"], cfg["slot"])
    assert lib.sg_step_drivers_policy(h, 1, None, 0) == STATE
    assert {"sg_set_driver_policy", "sg_driver_policy_actions", "sg_step_drivers_policy"} <= set(L.SYMBOLS) and L.ABI_VERSION == 7
    del keep_good, keep_empty
    for e_ in (eng, twin, plain):
        e_.close()


# ------------------------------------------------------------------------------------------------------------ 4. Python layers
@gpu
def test_vector_env_with_traffic(sga):
    """VectorScenarioEnv(drivers=..., traffic=...): thirty ticks with auto-reset against the engine-level loop of
    sg_driver_policy_actions, a host merge and sg_step_drivers, bit for bit on the state; shapes cover the caller's drivers only."""
    cfg = PS.column(2, mixed=True)
    cfg["scs"][0] = PS.cut_at(cfg["scs"][0], 1.25)  # a short episode: it ends (max_length) and starts anew within the run
    objs = _scenario_objects(cfg["scs"])
    drivers, traffic = [[5, 6], [5, 6]], [[1, 2, 3, 4], [1, 2, 3, 4]]
    kw = dict(timestep=PS.DT, n=8, terminal_conditions=["max_length"], max_steer=0.7, max_accel=5.0)
    with pytest.raises(ValueError):
        sga.VectorScenarioEnv(objs, traffic=traffic, **kw)
    with pytest.raises(ValueError):
        sga.VectorScenarioEnv(objs, drivers=drivers, traffic=[[1, 5], [1]], **kw)
    with pytest.raises(ValueError):
        sga.VectorScenarioEnv(objs, drivers=drivers, traffic=[[1]], **kw)
    tp = dict(v0=8.0, half=0.25)
    env = sga.VectorScenarioEnv(objs, drivers=drivers, traffic=traffic, traffic_params=tp, **kw)
    assert (env.n_drivers, env.n_traffic, env.engine._n_drv, env.engine._n_pol, env.engine._n_obs) == (4, 8, 12, 8, 4)
    assert env.reset().shape == (4, 2, 8, 8)
    # the same batch by hand: the caller's drivers first, the traffic behind them
    scen = np.array([0, 0, 1, 1] + [0] * 4 + [1] * 4, np.int32)
    slot = np.array([5, 6, 5, 6] + [1, 2, 3, 4] * 2, np.int32)
    packed = PS.pack(cfg["scs"])
    eng = sga.RolloutEngine(2, PS.COLUMN_E, timestep=PS.DT, terminal_conditions=["max_length"])
    eng.upload(packed)
    eng.set_road_networks([], np.full(2, -1, np.int32))
    eng.set_drivers(scen, slot)
    paths = [objs[r].entities[k].trajectory.data[:, 1:3] for r, k in zip(scen[4:], slot[4:])]
    eng.set_driver_policy(4 + np.arange(8), np.array([sga.idm_params(**tp)] * 8), paths)
    acts = PS.caller_actions(4, [], seed=8)
    restarted = np.zeros(2, bool)
    for k in range(30):
        obs, reward, done, info = env.step(acts[k])
        assert obs.shape == (4, 2, 8, 8) and reward.shape == (2,) and info["driver_flags"].shape == (4,) and info["driver_feat"].shape == (4, 3)
        merged = np.zeros((12, 2))
        merged[:4], merged[4:] = acts[k], eng.driver_policy_actions()[0]
        eng.step_drivers(merged[None], 1)
        want_done = (eng.terminal_flags() & 1) != 0
        assert np.array_equal(done, want_done)
        if want_done.any():
            eng.reset_scenarios(want_done)
            restarted |= want_done
        x, y = env.engine.state(raw=True), eng.state(raw=True)
        for key in x:
            assert np.array_equal(_bits(x[key]), _bits(y[key])), (k, key)
    assert restarted[0] and not restarted[1]
    moved = eng.state()["poses"][1, 1:5, 0] - packed.knots[packed.knot_off[PS.COLUMN_E + 1:PS.COLUMN_E + 5], 1]
    assert (moved > 5.0).all()  # (the traffic drove)
    env.close()
    eng.close()


@gpu
def test_vector_env_default_traffic_speed_and_no_traffic(sga):
    """The default v0 is the largest knot-to-knot speed of the recording, floored at 1 m/s; with traffic=None an episode is what
    it is today (a second environment given no such argument)."""
    cfg = PS.column(1, mixed=True)
    sc = cfg["scs"][0]
    sc["knots"][sc["knot_off"][7] + 1, 1] += 0.5 * PS.LENGTH  # the filler of slot 7 crawls at 0.5 m/s: below the floor
    objs = _scenario_objects(cfg["scs"])
    kw = dict(timestep=PS.DT, n=8, terminal_conditions=["max_length"], max_steer=0.7, max_accel=5.0)
    env = sga.VectorScenarioEnv(objs, drivers=[[5, 6]], traffic=[[1, 7]], **kw)
    # what the environment handed down, against an engine given the expected rows: the actions depend on v0 through (v / v0)^4
    k1 = sc["knots"][sc["knot_off"][1]:sc["knot_off"][2]]
    v1 = float(np.hypot(k1[1, 1] - k1[0, 1], k1[1, 2] - k1[0, 2]) / (k1[1, 0] - k1[0, 0]))
    assert abs(v1 - PS.V_START) < 1e-9
    packed = PS.pack(cfg["scs"])
    packed.kind[[1, 7]] = PS.KIND_AGENT_EXTERNAL
    packed.ctrl[[1, 7]] = packed.ctrl[5]
    eng = sga.RolloutEngine(1, PS.COLUMN_E, timestep=PS.DT, terminal_conditions=["max_length"])
    eng.upload(packed)
    eng.set_drivers([0, 0, 0, 0], [5, 6, 1, 7])
    paths = [objs[0].entities[k].trajectory.data[:, 1:3] for k in (1, 7)]
    eng.set_driver_policy([2, 3], np.array([sga.idm_params(v0=v1), sga.idm_params(v0=1.0)]), paths)
    got, want = env.engine.driver_policy_actions(), eng.driver_policy_actions()
    assert same(got, want) and np.isfinite(want[0]).all() and (eng.state()["ctrl_state"][0, [1, 7], 0] > 0.4).all()
    eng.set_driver_policy([2, 3], np.array([sga.idm_params(v0=v1), sga.idm_params(v0=0.5)]), paths)  # (without the floor: another answer)
    assert not same(got, eng.driver_policy_actions())
    eng.close()
    a = sga.VectorScenarioEnv(objs, drivers=[[5, 6]], traffic=None, **kw)
    b = sga.VectorScenarioEnv(objs, drivers=[[5, 6]], **kw)
    assert a.n_traffic == 0 and a.engine._n_pol == 0 and np.array_equal(a.reset(), b.reset())
    acts = PS.caller_actions(2, [], seed=9)
    for k in range(20):
        ra, rb = a.step(acts[k]), b.step(acts[k])
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[2], rb[2])
        x, y = a.engine.state(raw=True), b.engine.state(raw=True)
        for key in x:
            assert np.array_equal(_bits(x[key]), _bits(y[key])), (k, key)
    for e_ in (env, a, b):
        e_.close()
