"""The table rollout kernels store the pose, distance, presence and collision rows where the step loop is left, and the
velocity rows only in steps whose velocities can be seen afterwards (csrc/sgym_rollout.hpp, LATE).  What memory holds after a
call is what it held when every step stored every row: each scene below runs through the persistent launch, through chunk
launches (SG_QUEUE=0) and as the non-planar variant (SG_PLANAR=0), and EVERY scenario of it is compared with the CPU oracle
bit for bit -- poses, velocities, distances, presence, collision rows, controller state, ego metrics, events -- plus the raw
velocity rows of entities that have left the scene: they keep the velocity of the entity's last step in it.

The scenes aim at the ways a step loop is left and at the steps whose velocities stay visible:
  leavers     replay entities whose trajectory window ends (and others whose window begins) in the middle of a 16-step chunk,
              long before the call ends.  A trajectory has ONE window and the clock only moves forward, so within an episode no
              entity comes back; it does when the handle starts its next episode, which is the second half of the scene.
  ragged      tiles of 16 and 32 lanes whose scenarios have different lengths: they end at different steps of different chunks,
              one at step 1; the call is then resumed, so some scenarios -- and one whole wavefront -- are done when it starts.
  collision / ego_collision   the terminal condition fires in the middle of a chunk, well before max_length.
  replay_ego  a replay-agent ego (not a lane of the controller table: its metrics are taken from the step's velocities) beside
              PID lanes.
  resume      sg_step calls of odd lengths (force: done scenarios step on), and sg_rollout continued over several calls.
  one_step    sg_tick and one-step sg_step calls between rollouts: the next kernel starts from the rows the last one left.

test_scenes_do_what_they_are_for (CPU) runs the scenes through the oracle alone and asserts that those things do happen.
"""
import numpy as np
import pytest

DT = 1 / 30
CHUNK = 16
TAB = dict(tab_min_steps=1, chunk_steps=CHUNK)
MODES = {"queue": {}, "chunks": {"SG_QUEUE": "0"}, "nonplanar": {"SG_PLANAR": "0"}}
EXPECT = {"queue": "rollout_kernel_tabq_planar<", "chunks": "rollout_kernel_tab_planar<", "nonplanar": "rollout_kernel_tabq<"}


# ------------------------------------------------------------------------------------------------ scenes
def _base(R, E, T, seed, vanish=0.2, extent=None, ego="pid_sparse"):
    import scenario_gym_amd._lib as L
    from scenario_gym_amd import synthetic

    extent = 8.0 + 2.5 * np.sqrt(E) if extent is None else extent
    kind = L.KIND_AGENT_REPLAY if ego == "replay" else L.KIND_AGENT_PID
    p = synthetic.make_batch(R, E, n_steps=T + 40, ego_kind=kind, extent=extent, vanish_frac=vanish, seed=synthetic.SEED + seed)
    if ego == "pid_sparse":  # a PID ego in every fourth scenario (at most SG_TAB_LANES controlled lanes per wavefront)
        e = np.arange(R) * E
        p.kind[e[np.arange(R) % 4 != 0]] = L.KIND_AGENT_REPLAY
    return p


def _scene(name):
    """dict(packed, terminal, calls=[(entry, steps)], force): the calls run in order on one handle after the upload."""
    import scenario_gym_amd._lib as L

    if name in ("leavers-16", "leavers-64"):
        E = 12 if name.endswith("16") else 48
        return dict(packed=_base(16, E, 100, 1, vanish=0.5), terminal=["max_length"], calls=[("rollout", 100)], force=False)
    if name == "leavers-again":  # the handle's second episode: whoever left is back at the reset and leaves again
        return dict(packed=_base(16, 12, 100, 1, vanish=0.5), terminal=["max_length"], calls=[("rollout", 100), ("rollout", 100)],
                    force=False)
    if name in ("ragged-16", "ragged-32"):
        E, R = (12, 16) if name.endswith("16") else (24, 12)
        p = _base(R, E, 60, 2)
        ends = np.array([1, 5, 9, 7, 23, 40, 200, 11, 3, 200, 29, 37, 200, 13, 21, 35])[:R]  # steps; the first wavefront: all early
        p.length = p.t0 + (ends + 0.5) * DT
        return dict(packed=p, terminal=["max_length"], calls=[("rollout", 17), ("resume", 23), ("resume", 9)], force=False, ends=ends)
    if name in ("collision", "ego_collision"):
        p = _base(24, 12, 60, 3, extent=28.0)
        return dict(packed=p, terminal=["max_length", name], calls=[("rollout", 60)], force=False)
    if name == "replay_ego":
        R, E = 16, 12
        p = _base(R, E, 60, 4, ego="replay")
        n_knots = np.diff(p.knot_off).reshape(R, E)
        for r in range(0, R, 4):  # a PID agent on the first other slot whose trajectory spans the scenario
            s = 1 + int(np.argmax(n_knots[r, 1:] == n_knots[r, 0]))
            assert n_knots[r, s] == n_knots[r, 0]
            p.kind[r * E + s] = L.KIND_AGENT_PID
        return dict(packed=p, terminal=["max_length"], calls=[("rollout", 60)], force=False)
    if name == "resume-step":
        p = _base(16, 12, 60, 5)
        p.length = p.t0 + (np.array([200, 3, 200, 10, 26, 200, 200, 39] * 2) + 0.5) * DT  # (done scenarios step on)
        return dict(packed=p, terminal=["max_length"], calls=[("step", 7), ("step", 1), ("step", 13), ("step", 19)], force=True)
    if name == "resume-rollout":
        return dict(packed=_base(16, 12, 60, 6), terminal=["max_length"], calls=[("rollout", 7), ("resume", 1), ("resume", 13), ("resume", 19)],
                    force=False)
    if name == "one_step":  # nobody is done on the way (the scenarios are longer): the forced single steps are plain steps
        return dict(packed=_base(16, 12, 60, 7), terminal=["max_length"],
                    calls=[("rollout", 21), ("tick", 1), ("tick", 1), ("step", 1), ("resume", 15), ("step", 1), ("resume", 3)], force=False)
    raise ValueError(name)


SCENES = ["leavers-16", "leavers-64", "leavers-again", "ragged-16", "ragged-32", "collision", "ego_collision", "replay_ego",
          "resume-step", "resume-rollout", "one_step"]


def _episode(sc):
    """The calls of the handle's LAST episode (a "rollout" call resets) and their total number of steps."""
    calls = sc["calls"]
    first = max(i for i, c in enumerate(calls) if c[0] == "rollout") if any(c[0] == "rollout" for c in calls) else 0
    return calls[first:], sum(n for _, n in calls[first:])


def _oracle_all(O, sc):
    from scenario_gym_amd.engine import terminal_mask
    from scenario_gym_amd.packing import unpack_scenario

    p = sc["packed"]
    _, T = _episode(sc)
    out = []
    for r in range(p.n_scenarios):
        s = unpack_scenario(p, r)
        out.append(O.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], s["kind"], s["ego"], s["t0"], s["length"], DT,
                             terminal_mask=terminal_mask(sc["terminal"]), ctrl=s["ctrl"], max_steps=T, force_steps=sc["force"],
                             record=True, event_cap=64))
    return out


def _left_at(o):
    """Per entity: the last recorded step at which it was in the scene, for entities that are not at the end (else -1)."""
    here = ~np.isnan(o["poses"][:, :, 0])  # [steps + 1, E]
    last = here.shape[0] - 1 - np.argmax(here[::-1], axis=0)
    return np.where(here.any(axis=0) & ~here[-1], last, -1)


# ------------------------------------------------------------------------------------------------ CPU: the scenes bite
def test_scenes_do_what_they_are_for(oracle):
    import scenario_gym_amd._lib as L

    res = {n: (_scene(n), None) for n in SCENES}
    res = {n: (sc, _oracle_all(oracle, sc)) for n, (sc, _) in res.items()}
    for n in ("leavers-16", "leavers-64", "leavers-again"):
        sc, oo = res[n]
        T = _episode(sc)[1]
        left = np.concatenate([_left_at(o) for o in oo])
        mid = left[(left >= 1) & (left % CHUNK != CHUNK - 1) & (left % CHUNK != 0)]
        assert len(mid) >= 3 and (mid < T - 20).any(), (n, left)  # gone in the middle of a chunk, twenty steps and more before the end
        entered = np.concatenate([np.argmax(~np.isnan(o["poses"][:, :, 0]), axis=0) for o in oo])
        assert ((entered > 1) & (entered % CHUNK != 0)).any(), n  # ... and somebody comes in the middle of one
        assert all(o["n_steps"] == T for o in oo)
    for n in ("ragged-16", "ragged-32"):
        sc, oo = res[n]
        got = np.array([o["n_steps"] for o in oo])
        assert np.array_equal(got, np.minimum(sc["ends"], _episode(sc)[1])), (n, got)
        assert got.min() == 1 and (got[:4] < 17).all()  # one ends at step 1; the first four (a 16-lane wavefront) before the resumed calls
        assert len({int(g) // CHUNK for g in got}) >= 3 and (got % CHUNK != 0).all()
    for n in ("collision", "ego_collision"):
        sc, oo = res[n]
        p = sc["packed"]
        early = [o["n_steps"] for o, L_, t0 in zip(oo, p.length, p.t0) if o["is_done"] and o["final_t"] + DT <= L_]
        assert len(early) >= 2 and any(e % CHUNK not in (0, CHUNK - 1) for e in early), (n, early)  # the condition, not max_length
        assert any(not o["is_done"] for o in oo), n  # ... and not everywhere
        if n == "ego_collision":
            assert any(o["n_events"] > 0 and o["is_done"] for o in oo)
    sc, oo = res["replay_ego"]
    p = sc["packed"]
    assert (p.kind.reshape(p.n_scenarios, -1)[:, 0] == L.KIND_AGENT_REPLAY).all() and (p.kind == L.KIND_AGENT_PID).sum() == 4
    assert all(o["metric_ego_avg_speed"] > 0 and o["metric_ego_max_speed"] > 0 for o in oo)
    sc, oo = res["resume-step"]
    assert all(o["n_steps"] == 40 for o in oo) and sum(o["is_done"] for o in oo) >= 8  # forced on past their ends
    for n in ("resume-rollout", "one_step"):
        sc, oo = res[n]
        assert all(o["n_steps"] == _episode(sc)[1] and not o["is_done"] for o in oo), n


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def sga():
    import scenario_gym_amd as sga
    import scenario_gym_amd._lib as L

    L.load()
    return sga


def _play(eng, sc):
    names = []
    for entry, n in sc["calls"]:
        if entry == "rollout":
            eng.rollout(n)
        elif entry == "resume":
            eng.rollout_async(n, do_reset=False)
        elif entry == "step":
            eng.step(n, None)
        else:
            eng.tick(None, [0], nw=4, nh=4)
        eng.synchronize()
        names.append(eng.last_kernel())
    return names


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("scene", SCENES)
def test_final_state_equals_oracle(sga, oracle, monkeypatch, scene, mode):
    from oracle import check

    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    sc = _scene(scene)
    p = sc["packed"]
    R, E = p.n_scenarios, p.n_entities
    oo = _oracle_all(oracle, sc)
    eng = sga.RolloutEngine(R, E, timestep=DT, terminal_conditions=sc["terminal"], event_capacity=64)
    try:
        eng.set_tuning(**TAB)
        eng.upload(p)
        names = _play(eng, sc)
        tab_calls = [nm for (entry, _), nm in zip(sc["calls"], names) if entry != "tick"]
        assert all(EXPECT[mode] in nm for nm in tab_calls), (names, EXPECT[mode])  # (the kernels this file is about did run)
        st, raw = eng.state(), eng.state(raw=True)
        rows, events = eng.metrics()
        bad = {}
        for r in range(R):
            o = oo[r]
            b = check.compare_final(st, rows, events, r, o, E, event_cap=64, kind=p.kind[r * E:(r + 1) * E])
            if not np.array_equal(st["present"][r], ~np.isnan(o["poses"][-1][:, 0])):
                b.append("present")
            left = _left_at(o)
            for e in np.nonzero(left >= 1)[0]:  # gone: the rows keep the velocity of its last step in the scene
                if not check._bits(raw["vels"][r, e], o["vels"][left[e], e]):
                    b.append(f"velocity rows of entity {e}, gone after step {left[e]}")
            if b:
                bad[r] = b
        assert not bad, bad
    finally:
        eng.close()
