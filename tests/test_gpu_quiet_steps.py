"""Ego-quiet steps of the table rollout kernels (csrc/sgym_rollout.hpp QUIET, csrc/sgym_collide.hpp ego_near): a step in which no
body lies within the broad-phase reach of the ego, which is not the last step of a call and ends nobody's scenario, runs the
collision pass up to the box centres only -- the ego's row is 0, every other lane keeps the row of its last full pass until the
next one.  What memory holds after a call is what it held when every step ran the whole pass: each scene below runs through
the persistent launch, through chunk launches (SG_QUEUE=0) and as the non-planar variant (SG_PLANAR=0) -- the two scenes without
a controlled lane through rollout_kernel<G, 1, false, true>, the table kernel of batches that have none --, and EVERY scenario
of it is compared with the CPU oracle bit for bit -- poses, velocities, distances, presence, collision rows, controller state,
ego metrics, events and their order; one more run of every scene with SG_QUIET=0 must leave the same bytes.

The scenes (16 scenarios, at most 100 steps, chunks of 16 steps):
  tiles-16       four tiles of 16 lanes per wavefront: a tile is quiet while its neighbours are not -- the vote is the wavefront's.
  tile-64        one tile per wavefront, the shape of the headline workload.
  ragged         scenarios of different lengths, resumed over four calls: they end in the middle of a chunk while pairs that
                 do not involve the ego are in collision -- the step that ends a scenario runs the whole pass.
  replay_ego     a replay-agent ego (not a lane of the controller table) beside PID lanes.
  ego_collision  terminal conditions max_length and ego_collision: no step may be skipped.
  twins          two bit-identical static boxes on the ego's path and a third that touches them, quiet steps before (and, where
                 the ego gets past them, after) the encounter: owner mapping and event multiplicity right after skipped steps.
  absent_ego     replay-agent egos that are not in the scene.  An agent joins at the first step at or after which its
                 trajectory begins and stays (scenario_gym.py:240-244), so "absent" has two forms: absent in the reset state
                 and there from step 1 on, or -- its trajectory over when the scenario starts -- never there: every compare of
                 ego_near fails, every step but the last is skipped, and the others' rows must still be those of the last step.
  steps-force    sg_step calls of 1, 7 and 13 steps, forced on past the ends of the scenarios.
  steps-between  sg_tick and sg_step calls of 1, 7 and 13 steps between rollouts, nobody done.
  replay_only-16 / -64   replay-agent egos and no controlled lane at all: rollout_kernel<16 / 64, 1, false, true>.

test_scenes_bite (CPU) runs the scenes through the oracle alone and asserts that they can tell: in every scene the share of
steps with nothing inside the ego's reach lies strictly between 0.2 and 0.95, at least 100 such steps have a collision between
two others (stale rows would show at once if anything read them), there are at least 5 ego events, and at least 5 other lanes
are in collision at the final step.  Reach as in the kernel: own bounding-circle radius plus the tile's largest, about the box
centres (the kernel's adds a few millimetres of error margin; 1 cm here).
"""
import numpy as np
import pytest

import test_gpu_store_once as S

DT = S.DT
CHUNK = S.CHUNK
SCENES = ["tiles-16", "tile-64", "ragged", "replay_ego", "ego_collision", "twins", "absent_ego", "steps-force", "steps-between"]
REPLAY_SCENES = ["replay_only-16", "replay_only-64"]  # no controlled lane: the table kernel without a table
TWIN_A, TWIN_B, TWIN_C = 5, 9, 3  # the twins (the later slot owns the geometry) and the box that touches them


# ------------------------------------------------------------------------------------------------ scenes
def _replace_knots(p, new):
    """new: {flat entity index: [n, 7] knots} -- the other entities keep theirs."""
    n = len(p.knot_off) - 1
    parts = [new[e] if e in new else p.knots[p.knot_off[e]:p.knot_off[e + 1]] for e in range(n)]
    p.knots = np.concatenate(parts, axis=0)
    p.knot_off = np.concatenate([[0], np.cumsum([len(q) for q in parts])]).astype(np.int64)
    return p.validate()


def _pid_on_spanning_slot(p, every=4):
    """A PID agent on the first other slot whose trajectory spans the scenario, in every fourth scenario (as S replay_ego)."""
    import scenario_gym_amd._lib as L

    R, E = p.n_scenarios, p.n_entities
    n_knots = np.diff(p.knot_off).reshape(R, E)
    for r in range(0, R, every):
        s = 1 + int(np.argmax(n_knots[r, 1:] == n_knots[r, 0]))
        assert n_knots[r, s] == n_knots[r, 0]
        p.kind[r * E + s] = L.KIND_AGENT_PID


def _scene(name):
    """dict(packed, terminal, calls, force) as in test_gpu_store_once."""
    one = [("rollout", 100)]
    if name == "tiles-16":
        return dict(packed=S._base(16, 12, 100, 11), terminal=["max_length"], calls=one, force=False)
    if name == "tile-64":
        return dict(packed=S._base(16, 48, 100, 11), terminal=["max_length"], calls=one, force=False)
    if name == "ragged":
        p = S._base(16, 12, 100, 11)
        ends = np.array([1, 45, 69, 37, 23, 40, 200, 51, 3, 200, 29, 77, 200, 83, 61, 35])
        p.length = p.t0 + (ends + 0.5) * DT
        return dict(packed=p, terminal=["max_length"], calls=[("rollout", 37), ("resume", 23), ("resume", 9), ("resume", 29)], force=False,
                    ends=ends)
    if name == "replay_ego":
        p = S._base(16, 12, 100, 11, ego="replay")
        _pid_on_spanning_slot(p)
        return dict(packed=p, terminal=["max_length"], calls=one, force=False)
    if name == "ego_collision":
        return dict(packed=S._base(16, 12, 100, 3, extent=24.0), terminal=["max_length", "ego_collision"], calls=one, force=False)
    if name == "twins":
        p = S._base(16, 12, 100, 12)
        E, new = p.n_entities, {}
        for r in range(p.n_scenarios):
            k = p.knots[p.knot_off[r * E]:p.knot_off[r * E + 1]]  # the ego's trajectory: where it is 30 + 3 r steps in
            tm = p.t0[r] + (30 + 3 * r) * DT
            x, y, h = (np.interp(tm, k[:, 0], k[:, c]) for c in (1, 2, 4))
            box = np.zeros((1, 7))
            box[0, 0], box[0, 1], box[0, 2], box[0, 4] = p.t0[r], x, y, h + 0.3
            new[r * E + TWIN_A], new[r * E + TWIN_B] = box.copy(), box.copy()
            side = box.copy()  # 1.5 m to the left of them: the 2 m wide boxes overlap
            side[0, 1] += 1.5 * np.cos(h + 0.3 + np.pi / 2)
            side[0, 2] += 1.5 * np.sin(h + 0.3 + np.pi / 2)
            new[r * E + TWIN_C] = side
        return dict(packed=_replace_knots(p, new), terminal=["max_length"], calls=one, force=False)
    if name == "absent_ego":
        p = S._base(16, 12, 100, 11, ego="replay")
        _pid_on_spanning_slot(p)
        E, new = p.n_entities, {}
        for r in range(p.n_scenarios):
            k = p.knots[p.knot_off[r * E]:p.knot_off[r * E + 1]]
            if r % 4 == 1:  # the trajectory is over when the scenario starts: never in the scene
                new[r * E] = k[k[:, 0] < 0.3].copy()
                p.t0[r] = 0.5
            elif r % 4 == 2:  # the trajectory begins half a second in: absent in the reset state, there from step 1 on
                new[r * E] = k[k[:, 0] > p.t0[r] + 0.5].copy()
        return dict(packed=_replace_knots(p, new), terminal=["max_length"], calls=one, force=False)
    if name == "steps-force":
        p = S._base(16, 12, 100, 11)
        p.length = p.t0 + (np.array([200, 3, 200, 10, 26, 200, 200, 39] * 2) + 0.5) * DT  # (done scenarios step on)
        return dict(packed=p, terminal=["max_length"], calls=[("step", n) for n in (7, 1, 13, 7, 13, 1, 13, 7, 13, 13)], force=True)
    if name == "steps-between":
        return dict(packed=S._base(16, 12, 100, 11), terminal=["max_length"],
                    calls=[("rollout", 21), ("tick", 1), ("step", 7), ("resume", 15), ("step", 13), ("tick", 1), ("resume", 23), ("step", 1),
                           ("resume", 11)], force=False)
    if name in REPLAY_SCENES:
        E = 12 if name.endswith("16") else 48
        return dict(packed=S._base(16, E, 100, 11, ego="replay"), terminal=["max_length"], calls=one, force=False,
                    expect=f"rollout_kernel<{16 if E == 12 else 64}, 1, false, true>")
    raise ValueError(name)


_ORACLE = {}


def _oracle_of(O, name):
    """(scene, oracle results of all its scenarios): computed once, shared by the tests, never changed."""
    if name not in _ORACLE:
        sc = _scene(name)
        _ORACLE[name] = (sc, S._oracle_all(O, sc))
    return _ORACLE[name]


# ------------------------------------------------------------------------------------------------ CPU: the scenes bite
def _quiet_steps(p, r, o):
    """Per executed step of scenario r: is nothing inside the ego's reach?  And: are two others in collision?"""
    from scenario_gym_amd.packing import unpack_scenario

    s = unpack_scenario(p, r)
    bb = np.asarray(s["bbox"], float).reshape(-1, 4)  # width, length, centre x, centre y
    rad = 0.5 * np.hypot(bb[:, 0], bb[:, 1])
    e = int(s["ego"])
    P = o["poses"][1:]
    h = P[:, :, 3]
    cx = P[:, :, 0] + bb[:, 2] * np.cos(h) - bb[:, 3] * np.sin(h)
    cy = P[:, :, 1] + bb[:, 2] * np.sin(h) + bb[:, 3] * np.cos(h)
    d = np.hypot(cx - cx[:, e:e + 1], cy - cy[:, e:e + 1])
    d[:, e] = np.nan
    near = (np.nan_to_num(d, nan=1e9) <= rad[e] + rad.max() + 0.01).any(axis=1)  # (an absent ego: NaN, nobody is near)
    coll = np.asarray(o["coll"]).reshape(len(o["poses"]), len(bb), -1)[1:].any(axis=-1)
    return ~near, np.delete(coll, e, axis=1)


@pytest.mark.parametrize("scene", SCENES + REPLAY_SCENES)
def test_scenes_bite(oracle, scene):
    sc, oo = _oracle_of(oracle, scene)
    p = sc["packed"]
    n_quiet = n_steps = mixed = events = final = 0
    quiet_of = []
    for r, o in enumerate(oo):
        quiet, others = _quiet_steps(p, r, o)
        quiet_of.append(quiet)
        n_quiet += int(quiet.sum())
        n_steps += len(quiet)
        mixed += int((quiet & others.any(axis=1)).sum())
        events += int(o["n_events"])
        final += int(others[-1].sum())
    share = n_quiet / n_steps
    print(f"{scene}: quiet share {share:.3f}, quiet steps with a collision between others {mixed}, ego events {events}, "
          f"other lanes in collision at the final step {final}")
    assert 0.2 < share < 0.95, share
    assert mixed >= 100 and events >= 5 and final >= 5, (mixed, events, final)
    if scene == "ragged":
        got = np.array([o["n_steps"] for o in oo])
        assert np.array_equal(got, np.minimum(sc["ends"], S._episode(sc)[1])), got
        mid = [r for r, o in enumerate(oo) if o["is_done"] and got[r] % CHUNK not in (0, CHUNK - 1)
               and np.delete(np.asarray(o["coll"])[-1].reshape(p.n_entities, -1).any(axis=-1), 0).any()]
        assert len(mid) >= 4, mid  # ended mid-chunk with others in collision
    if scene == "ego_collision":
        assert sum(o["is_done"] and o["n_events"] > 0 for o in oo) >= 3 and any(not o["is_done"] for o in oo)
    if scene == "twins":
        before = around = 0
        for r, o in enumerate(oo):
            other = np.asarray(o["ev_other"])
            assert not (other == TWIN_A).any(), r  # the geometry belongs to its last owner ...
            hit = np.nonzero(other == TWIN_B)[0]
            assert len(hit) == 2 and TWIN_C in other, (r, other)  # ... which is listed once per twin
            k = int(round((o["ev_t"][hit[0]] - p.t0[r]) / DT))  # the step of the encounter (rows of quiet_of: step - 1)
            before += bool(quiet_of[r][:k - 1].any())
            around += bool(quiet_of[r][:k - 1].any() and quiet_of[r][k:].any())
        print(f"twins: quiet steps before the encounter in {before} scenarios, before and after it in {around}")
        assert before >= 8 and around >= 3, (before, around)
    if scene in REPLAY_SCENES:
        import scenario_gym_amd._lib as L

        assert set(p.kind.tolist()) <= {L.KIND_REPLAY, L.KIND_AGENT_REPLAY}, set(p.kind.tolist())  # nobody for a controller table
    if scene == "absent_ego":
        here = [~np.isnan(o["poses"][:, 0, 0]) for o in oo]
        assert sum(not h.any() for h in here) == 4 and sum((not h[0]) and h[1:].all() for h in here) == 4
    if scene == "steps-force":
        assert all(o["n_steps"] == 88 for o in oo) and sum(o["is_done"] for o in oo) >= 8
    if scene == "steps-between":
        assert all(o["n_steps"] == 93 and not o["is_done"] for o in oo)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def sga():
    import scenario_gym_amd as sga
    import scenario_gym_amd._lib as L

    L.load()
    return sga


def _run(sga, sc, mode):
    """The scene's calls on a fresh handle: (mismatches against the oracle per scenario, bytes of everything read back)."""
    p = sc["packed"]
    R, E = p.n_scenarios, p.n_entities
    eng = sga.RolloutEngine(R, E, timestep=DT, terminal_conditions=sc["terminal"], event_capacity=64)
    try:
        eng.set_tuning(**S.TAB)
        eng.set_slicing(False)  # (a batch without controlled lanes would be cut along the time axis: not the kernels of this file)
        eng.upload(p)
        names = S._play(eng, sc)
        tab_calls = [nm for (entry, _), nm in zip(sc["calls"], names) if entry != "tick"]
        expect = sc.get("expect", S.EXPECT.get(mode))
        assert all(expect in nm for nm in tab_calls), (names, expect)  # (the kernels this file is about did run)
        st, raw = eng.state(), eng.state(raw=True)
        rows, events = eng.metrics()
    finally:
        eng.close()
    as_bytes = lambda d: (b"".join(np.ascontiguousarray(d[k]).tobytes() for k in sorted(d)) if isinstance(d, dict)
                          else np.ascontiguousarray(d).tobytes())
    blob = b"".join(as_bytes(d) for d in (st, raw, rows, events))
    return st, rows, events, blob


def _check(sga, oracle, monkeypatch, scene, mode):
    from oracle import check

    sc, oo = _oracle_of(oracle, scene)
    p = sc["packed"]
    E = p.n_entities
    monkeypatch.delenv("SG_QUIET", raising=False)
    st, rows, events, blob = _run(sga, sc, mode)
    bad = {}
    for r, o in enumerate(oo):
        b = check.compare_final(st, rows, events, r, o, E, event_cap=64, kind=p.kind[r * E:(r + 1) * E])
        if not np.array_equal(st["present"][r], ~np.isnan(o["poses"][-1][:, 0])):
            b.append("present")
        if b:
            bad[r] = b
    assert not bad, bad
    monkeypatch.setenv("SG_QUIET", "0")  # every step runs the whole pass: the same bytes
    assert _run(sga, sc, mode)[3] == blob


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(S.MODES))
@pytest.mark.parametrize("scene", SCENES)
def test_quiet_steps_equal_oracle(sga, oracle, monkeypatch, scene, mode):
    for k, v in S.MODES[mode].items():
        monkeypatch.setenv(k, v)
    _check(sga, oracle, monkeypatch, scene, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", REPLAY_SCENES)
def test_quiet_steps_without_controlled_lanes(sga, oracle, monkeypatch, scene):
    _check(sga, oracle, monkeypatch, scene, None)
