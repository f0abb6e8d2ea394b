"""Device snapshots: sg_snapshot_create / _save / _restore / _bytes / _destroy (snapshot_copy_kernel) and the Python layers over them.

Every expectation comes from an uninterrupted TWIN handle that runs existing code paths only, never from the code under test:
twin A uploads, steps K, then steps M; B uploads, steps K, saves, is disturbed (J steps with other actions and a reset of some
scenarios), restores, then steps M.  Right after the restore everything readable of B equals what was read at the save, and after
the M steps it equals A, bit for bit.  Scenarios are independent, so a masked case composes its expectation per scenario from twins.

1. every kernel family: one row per family and entry point of test_gpu_variants.VARIANTS at the family's smallest shape, plus rows
   at E = 100 (two wavefronts per scenario), E = 300 (eight: last_row_hi) and E = 600 (the multi-kernel step)
2. masks inside one 64-slot block at E = 3 (16 scenarios per block): save and restore masks that differ, host and device masks
3. pedestrian noise: the stream position and the counter-based generator
4. RSS records and the pose record
5. caller-run poses
6. the device tick: drivers, traffic policy, progress reward, through an auto-reset; a snapshot taken before the first tick
7. stream order: save, step, restore, step queued back to back with a device mask made by torch
8. VectorScenarioEnv.save_state / restore_state in an MPC-shaped loop, default path, driver list and device_tick
9. lifecycle and refusals
(The CPU side -- the state inventory, the binding, the kernel's resources -- is tests/test_snapshot_inventory.py.)
"""
import ctypes as C

import numpy as np
import pytest

import policy_scenes as PS
import test_episode as TE
import test_gpu_variants as V
from test_drivers import _assert_same, _scenario_objects, _snapshot
from test_gpu_variants import sga  # noqa: F401  (the fixture)

gpu = pytest.mark.gpu
K, J, M = 7, 6, 8
DT = V.DT


# ------------------------------------------------------------------------------------------------------------------ what is compared
def _readable(eng, rss=False, record=0):
    """Everything a caller can read of a handle: _snapshot of test_drivers.py, the collision points, and where they apply the RSS
    records and the pose record."""
    snap = _snapshot(eng)
    snap["collision_points"] = eng.collision_points()
    if rss:
        for name, v in zip(("rss_lon", "rss_lat", "rss_codes", "rss_safe"), eng.rss()):
            snap[name] = np.asarray(v)
    if record:
        snap["rec_t"], snap["rec_poses"] = eng.record(record)
    return snap


def _of_scenario(snap, r, R):
    """The part of a _readable that belongs to scenario r."""
    out = {}
    for k, a in snap.items():
        if k.startswith("event_") or k == "collision_points":
            out[k] = a[snap["event_scenario"] == r]
        elif k == "scen":
            out[k] = a.reshape(R, -1)[r]
        elif k in ("rec_t", "rec_poses"):
            out[k] = a[:, r]
        else:
            out[k] = a[r]
    return out


def _assert_scenarios(got, want_of, R, what):
    """got: a _readable; want_of[r]: the _readable scenario r is expected to equal."""
    for r in range(R):
        _assert_same(_of_scenario(got, r, R), _of_scenario(want_of[r], r, R), f"{what}, scenario {r}")


def _actions(n, R, seed):
    from scenario_gym_amd import synthetic

    return synthetic.make_actions(n, R, seed=synthetic.SEED + seed)


def _disturb(eng, R, other):
    """J steps with other actions, a reset of some scenarios, two steps more."""
    eng.step(J, other[:J])
    eng.reset_scenarios((np.arange(R) % 3 == 1).astype(np.uint8))
    eng.step(2, other[J:J + 2])


# ------------------------------------------------------------------------------------------------------------ 1. every kernel family
def _family_rows():
    """One row per (family, entry point) of VARIANTS at the family's smallest shape, and the wider shapes of the general families.
    The two slice families are left out: a sliced call always begins with a reset, so no saved state ever reaches them."""
    best = {}
    for r in V.VARIANTS:
        if r["family"] in ("slice", "slice_tab"):
            continue
        key = (r["family"], r["recipe"] if r["family"] == "wide" else "", r["entry"])
        if key not in best or r["E"] < best[key]["E"]:
            best[key] = r
    rows = list(best.values())
    have = {r["id"] for r in rows}
    wider = {100: ("plain", "ped", "rss", "tab_rows"), 300: ("plain", "rss")}
    rows += [r for r in V.VARIANTS if r["id"] not in have and r["family"] in wider.get(r["E"], ())]
    return rows


FAMILY_ROWS = _family_rows()


def test_family_rows_cover_the_shapes():
    """(CPU) the selection holds EP = 4, two and eight wavefronts per scenario and the multi-kernel step, and every entry point."""
    assert {3, 100, 300, 600} <= {r["E"] for r in FAMILY_ROWS}
    assert {r["entry"] for r in FAMILY_ROWS} == {"rollout", "step", "tick"}
    fams = {r["family"] for r in V.VARIANTS} - {"slice", "slice_tab"}
    assert {r["family"] for r in FAMILY_ROWS} == fams and len(fams) >= 20


def _prepare(sga, row, inputs, record=0):  # noqa: F811
    """A handle with the row's knobs and batch, as test_gpu_variants._run sets it up, before any step."""
    packed, nets, net_of, model_of, _ = inputs
    eng = sga.RolloutEngine(row["R"], row["E"], timestep=DT, terminal_conditions=V._terminal(row), event_capacity=64, record_capacity=record)
    if row["tuning"]:
        eng.set_tuning(**row["tuning"])
    eng.set_slicing(row["slicing"])
    eng.set_rss(row["rss"])
    if model_of is not None:
        eng.set_ped_models(V.MODELS, model_of)
    eng.upload(packed)
    if nets is not None:
        eng.set_road_networks(nets, net_of)
    return eng


def _advance(eng, entry, acts, first=False):
    """len(acts) steps by the row's entry point; `first`: the call that opens the run (sg_rollout resets)."""
    n = len(acts)
    if entry == "step":
        eng.step(n, acts)
    elif entry == "tick":
        for a in acts:
            eng.tick(a, [0], nw=4, nh=4)
    elif first:
        eng.rollout(n)
    else:
        eng.rollout_async(n, do_reset=False)
    eng.synchronize()


def _twin_run(sga, row, prepare=_prepare, record=0, before_save=None, disturb=_disturb):  # noqa: F811
    """The pattern of the module docstring on one row; returns (what B read at the save, what A and B read at the end)."""
    row = dict(row, T=K + J + M + 4)  # (the batch outlasts every run)
    inputs = V._stage_inputs(row)
    R = row["R"]
    acts, other = _actions(K + M, R, 1), _actions(J + 2, R, 2)
    read = lambda e: _readable(e, row["rss"], record)  # noqa: E731
    A, B = prepare(sga, row, inputs, record), prepare(sga, row, inputs, record)
    try:
        for e in (A, B):
            if before_save:
                before_save(e, 0)
            _advance(e, row["entry"], acts[:K], first=True)
        snap = B.snapshot()
        assert snap.nbytes > 0
        at_save = read(B)
        _assert_same(at_save, read(A), "at the save")
        if before_save:
            before_save(B, 1)
        disturb(B, R, other)
        assert not np.array_equal(_snapshot(B)["t"], at_save["t"])  # (the restore has something to undo)
        snap.restore()
        _assert_same(read(B), at_save, "right after the restore")
        for e in (A, B):
            _advance(e, row["entry"], acts[K:])
        if row.get("expect"):  # (the rows of VARIANTS: the continuation really reached the family)
            assert B.last_kernel() == row["expect"] and A.last_kernel() == row["expect"]
        a, b = read(A), read(B)
        _assert_same(b, a, "after the continuation")
        if row["entry"] != "rollout":  # (sg_rollout lets a finished scenario sit the steps out: an ego off the road from the start)
            assert not np.array_equal(a["t"], at_save["t"])  # the continuation did step
        return at_save, a
    finally:
        A.close()
        B.close()


@gpu
@pytest.mark.parametrize("row", FAMILY_ROWS, ids=[r["id"] for r in FAMILY_ROWS])
def test_restore_then_continue_equals_the_twin(sga, monkeypatch, row):  # noqa: F811
    """Save, disturb, restore and continue by the row's entry point: the continuation reaches the row's family and B equals A."""
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    _twin_run(sga, row)


# ---------------------------------------------------------------------------------------------------------------------- 2. masks
MASK_R, MASK_E = 32, 3  # EP = 4: two 64-slot blocks of 16 scenarios each
_ALT = np.arange(MASK_R) % 2 == 0
MASKS = {
    "subset": (_ALT, np.arange(MASK_R) % 4 == 0),
    "superset": (_ALT, _ALT | (np.arange(MASK_R) % 3 == 0)),
    "zeros": (np.zeros(MASK_R, bool), np.zeros(MASK_R, bool)),
    "ones": (np.ones(MASK_R, bool), np.ones(MASK_R, bool)),
    "save_none_restore_odd": (np.zeros(MASK_R, bool), ~_ALT),
}


def _mask_engine(sga):  # noqa: F811
    row = dict(recipe="vehicle", R=MASK_R, E=MASK_E, T=K + J + M + 4, road=False)
    eng = sga.RolloutEngine(MASK_R, MASK_E, timestep=DT, terminal_conditions=["max_length"], event_capacity=64)
    eng.upload(V._stage_inputs(row)[0])
    return eng


@pytest.fixture(scope="module")
def mask_twins(sga):  # noqa: F811
    """What uninterrupted handles read: at the reset (s0), after K steps (sk), and at the end of the three histories a scenario of the
    masked handle can have -- saved after K and restored (K + M steps), never saved but restored (the rows of the create: M steps
    from the reset), not restored (K + J + M steps)."""
    a1, a2, a3 = _actions(K, MASK_R, 3), _actions(J, MASK_R, 4), _actions(M, MASK_R, 5)
    out = dict(acts=(a1, a2, a3))
    A, A0, Cc = _mask_engine(sga), _mask_engine(sga), _mask_engine(sga)
    out["s0"] = _readable(A)
    A.step(K, a1)
    out["sk"] = _readable(A)
    A.step(M, a3)
    out["saved"] = _readable(A)
    A0.step(M, a3)
    out["created"] = _readable(A0)
    Cc.step(K, a1)
    Cc.step(J, a2)
    out["skj"] = _readable(Cc)
    Cc.step(M, a3)
    out["untouched"] = _readable(Cc)
    for e in (A, A0, Cc):
        e.close()
    return out


@gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", sorted(MASKS))
def test_masks_inside_one_block(sga, mask_twins, name, where):  # noqa: F811
    import torch

    save_mask, restore_mask = MASKS[name]
    a1, a2, a3 = mask_twins["acts"]
    give = (lambda m: torch.as_tensor(m.astype(np.uint8), device="cuda:0")) if where == "device" else (lambda m: m if name == "subset" else m.astype(np.uint8))
    B = _mask_engine(sga)
    try:
        snap = B.snapshot()  # (every row: the reset state)
        B.step(K, a1)
        snap.save(give(save_mask))
        B.step(J, a2)
        # the handle: untouched by the save
        _assert_same(_readable(B), mask_twins["skj"], "the save left the handle alone")
        snap.restore(give(restore_mask))
        want = [(mask_twins["sk"] if save_mask[r] else mask_twins["s0"]) if restore_mask[r] else mask_twins["skj"] for r in range(MASK_R)]
        _assert_scenarios(_readable(B), want, MASK_R, "right after the masked restore")
        B.step(M, a3)
        want = [(mask_twins["saved"] if save_mask[r] else mask_twins["created"]) if restore_mask[r] else mask_twins["untouched"]
                for r in range(MASK_R)]
        _assert_scenarios(_readable(B), want, MASK_R, "after the continuation")
        # the snapshot: only the masked rows were ever written
        snap.restore()
        want = [mask_twins["sk"] if save_mask[r] else mask_twins["s0"] for r in range(MASK_R)]
        _assert_scenarios(_readable(B), want, MASK_R, "the second, full restore")
    finally:
        B.close()


# ------------------------------------------------------------------------------------------------------------- 3. pedestrian noise
@gpu
@pytest.mark.parametrize("mode", ["stream", "device"])
def test_pedestrian_noise_continues_where_it_was_saved(sga, mode):  # noqa: F811
    """A PID car in a social-force crowd with noise: the disturbance consumes variates, the continuation equals the twin's."""
    row = V._row("ped", "mixed", 12, 6, "step", None)
    normals = np.random.default_rng(5).standard_normal((row["R"], 2 * row["E"] * (K + J + M + 8)))

    def prepare(sga_, row_, inputs, record):
        packed = inputs[0]
        eng = sga_.RolloutEngine(row_["R"], row_["E"], timestep=DT, terminal_conditions=["max_length"], event_capacity=64)
        eng.set_tuning(**row_["tuning"])
        eng.set_ped_noise(mode, 0.3, 0.2, normals=normals if mode == "stream" else None, seed=77)
        eng.upload(packed)
        return eng

    at_save, end = _twin_run(sga, row, prepare=prepare)
    if mode == "stream":
        assert (at_save["noise_pos"] > 0).all() and (end["noise_pos"] > at_save["noise_pos"]).all()


# --------------------------------------------------------------------------------------------- 4. RSS records and the pose record
@gpu
@pytest.mark.parametrize("E", [6, 300])
def test_rss_records_and_the_pose_record(sga, E):  # noqa: F811
    """record_capacity > 0 and sg_set_rss: the disturbance writes record rows and RSS history the restore takes away again."""
    R = 8 if E == 6 else 3
    row = V._row("rss", "vehicle", E, R, "step", None, rss=True)
    cap = K + J + M + 6
    at_save, end = _twin_run(sga, row, record=cap)
    assert (at_save["rss_codes"] >= 0).any()  # (the callback did run)
    scen = np.frombuffer(at_save["scen"].tobytes(), sga.engine.SCEN_DTYPE)
    assert (scen["rec_rows"] == K + 1).all()
    scen = np.frombuffer(end["scen"].tobytes(), sga.engine.SCEN_DTYPE)
    assert (scen["rec_rows"] == K + M + 1).all()  # (the rows the disturbance wrote are gone)


# ------------------------------------------------------------------------------------------------------------ 5. caller-run poses
@gpu
def test_caller_run_poses(sga):  # noqa: F811
    """An SG_KIND_AGENT_EXTERNAL slot keeps the pose of sg_set_external_poses until another is set: it is state."""
    import scenario_gym_amd._lib as L

    row = V._row("plain", "vehicle", 6, 8, "step", None)
    R, E = row["R"], row["E"]
    poses = np.full((2, R, E, 6), np.nan)
    poses[0, :, 1] = (3.0, -4.0, 0.0, 0.25, 0.0, 0.0)
    poses[1, :, 1] = (-7.5, 2.0, 0.0, 1.5, 0.0, 0.0)

    def prepare(sga_, row_, inputs, record):
        packed = inputs[0]
        packed.kind[np.arange(R) * E + 1] = L.KIND_AGENT_EXTERNAL
        eng = sga_.RolloutEngine(R, E, timestep=DT, terminal_conditions=["max_length"], event_capacity=64)
        eng.upload(packed)
        return eng

    at_save, end = _twin_run(sga, row, prepare=prepare, before_save=lambda eng, which: eng.set_external_poses(poses[which]))
    assert (end["poses"][:, 1, 0] == 3.0).any()  # (the slot is where the pose set before the save put it)


# ------------------------------------------------------------------------------------------------------------- 6. the device tick
def _ticks(eng, acts, rules, n):
    return [TE._read(eng, TE._tick(eng, a, rules), n) for a in acts]


@gpu
def test_device_tick_through_an_auto_reset(sga):  # noqa: F811
    """The column with the traffic policy and the progress reward, scenario 0 cut at 1.25 s (12 ticks): save mid-episode, tick on
    through its auto-reset, restore, tick.  Every array of the view equals the twin's; progress, return and length continue."""
    cfg = TE.column_batch()
    rules = TE.RULES["defaults"]
    n = len(cfg["scen"])
    acts, other = TE.batch_actions(cfg, seed=2), TE.batch_actions(cfg, seed=9)
    A, B = TE._engine(sga, cfg), TE._engine(sga, cfg)
    try:
        early = B.snapshot()  # before the first tick ever
        va, vb = _ticks(A, acts[:K], rules, n), _ticks(B, acts[:K], rules, n)
        TE._same_view(vb[-1], va[-1], "before the save")
        snap = B.snapshot()
        at_save = _readable(B)
        seen = _ticks(B, other[:J + 2], rules, n)
        assert any(v["reset_mask"][0] for v in seen) and not any(v["reset_mask"][1] for v in seen)  # (through an auto-reset)
        snap.restore()
        _assert_same(_readable(B), at_save, "right after the restore")
        va, vb = _ticks(A, acts[K:K + M], rules, n), _ticks(B, acts[K:K + M], rules, n)
        for k, (x, y) in enumerate(zip(vb, va)):
            TE._same_view(x, y, f"tick {k} after the restore")
        TE._same_state(A, B, "after the restore")
        assert (vb[0]["drv_progress"] != 0.0).any()  # the saved arclength difference, not the 0 of a first tick
        assert (vb[0]["ep_length"] == K + 1).all() and not np.array_equal(vb[0]["ep_return"], vb[0]["drv_reward"])
        # the snapshot of before the first tick: the accounting of a fresh episode
        early.restore()
        fresh = TE._engine(sga, cfg)
        try:
            vf, vb = _ticks(fresh, acts[:3], rules, n), _ticks(B, acts[:3], rules, n)
            for k, (x, y) in enumerate(zip(vb, vf)):
                TE._same_view(x, y, f"tick {k} from the snapshot of before the first tick")
            TE._same_state(fresh, B, "from the early snapshot")
            assert (vb[0]["ep_length"] == 1).all() and not vb[0]["drv_progress"].any()
        finally:
            fresh.close()
    finally:
        A.close()
        B.close()


# -------------------------------------------------------------------------------------------------------------- 7. stream order
@gpu
def test_queued_back_to_back_equals_waited_for(sga):  # noqa: F811
    """save -> steps -> save of a second snapshot -> restore -> steps with no wait in between and a device mask torch makes just before
    and overwrites just after: the same as with a wait after every call.  The second snapshot holds what the handle held then."""
    import torch

    row = dict(recipe="pid", R=16, E=6, T=K + J + M + 4, road=False)
    packed = V._stage_inputs(row)[0]
    R = row["R"]
    alt = np.arange(R) % 2 == 0

    def run(wait):
        eng = sga.RolloutEngine(R, row["E"], timestep=DT, terminal_conditions=["max_length"], event_capacity=64)
        eng.set_tuning(**V.TAB)  # (the table path: its pre-pass runs on the handle's second stream)
        eng.upload(packed)
        s1, s2 = eng.snapshot(), eng.snapshot()
        eng.synchronize()
        sync = eng.synchronize if wait else (lambda: None)
        eng.rollout_async(K, do_reset=False)
        sync()
        m = torch.zeros(R, dtype=torch.uint8, device="cuda:0")
        m[::2] = 1
        s1.save(m)
        sync()
        eng.rollout_async(J, do_reset=False)
        sync()
        s2.save()
        sync()
        s1.restore(m)
        m.zero_()  # (ordered behind the restore: ordered_with_torch)
        sync()
        eng.rollout_async(M, do_reset=False)
        eng.synchronize()
        end = _readable(eng)
        s1.save()  # operations on the first snapshot leave the second alone
        s2.restore()
        eng.synchronize()
        mid = _readable(eng)
        eng.close()
        return end, mid

    end_q, mid_q = run(False)
    end_w, mid_w = run(True)
    _assert_same(end_q, end_w, "queued against waited for")
    _assert_same(mid_q, mid_w, "the second snapshot, queued against waited for")
    # ... and both are what twins compute: K + M steps where the mask is set, K + J + M where it is not; K + J in the second snapshot
    twins = {}
    for name, n in (("saved", K + M), ("untouched", K + J + M), ("mid", K + J)):
        eng = sga.RolloutEngine(R, row["E"], timestep=DT, terminal_conditions=["max_length"], event_capacity=64)
        eng.set_tuning(**V.TAB)
        eng.upload(packed)
        for part in ((K, M) if name == "saved" else (K, J, M) if name == "untouched" else (K, J)):
            eng.rollout_async(part, do_reset=False)
        eng.synchronize()
        twins[name] = _readable(eng)
        eng.close()
    _assert_scenarios(end_q, [twins["saved"] if alt[r] else twins["untouched"] for r in range(R)], R, "queued against the twins")
    _assert_same(mid_q, twins["mid"], "the second snapshot against its twin")


# ----------------------------------------------------------------------------------------------------------- 8. VectorScenarioEnv
def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same_step(got, want, what):
    (o1, r1, d1, i1), (o2, r2, d2, i2) = got, want
    assert _np(o1).tobytes() == _np(o2).tobytes() and _np(o1).shape == _np(o2).shape, (what, "obs")
    assert _np(r1).tobytes() == _np(r2).tobytes() and _np(d1).tobytes() == _np(d2).tobytes(), (what, "reward / done")
    assert set(i1) == set(i2)
    for key in i1:
        assert _np(i1[key]).tobytes() == _np(i2[key]).tobytes(), (what, key)


@gpu
@pytest.mark.parametrize("path", ["ego", "drivers", "device_tick"])
def test_vector_env_planning_loop(sga, path):  # noqa: F811
    """save_state; three candidate action sets, each stepped 4 ticks after a restore_state; restore_state; step the chosen one:
    observations, rewards, dones and infos equal a twin environment that only ever took the chosen actions.  Scenario 0 is cut at
    1.25 s, so candidates and chosen steps cross an auto-reset."""
    import torch

    cfg = PS.column(2, mixed=True)
    cfg["scs"][0] = PS.cut_at(cfg["scs"][0], 1.25)
    objs = _scenario_objects(cfg["scs"])
    kw = dict(timestep=PS.DT, n=8, terminal_conditions=["max_length"], max_steer=0.7, max_accel=5.0)
    n_act = 2
    if path != "ego":
        kw.update(drivers=[[5, 6], [5, 6]], traffic=[[1, 2, 3, 4], [1, 2, 3, 4]], traffic_params=dict(v0=8.0, half=0.25), driver_progress=1.0,
                  torch_obs=path == "device_tick", device_tick=path == "device_tick")
        n_act = 4
    env, twin = sga.VectorScenarioEnv(objs, **kw), sga.VectorScenarioEnv(objs, **kw)
    try:
        acts = PS.caller_actions(n_act, [], seed=11)
        acts[..., 0] += 1.0
        cands = [PS.caller_actions(n_act, [], seed=20 + c) for c in range(3)]
        give = (lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")) if path == "device_tick" else (lambda a: a)
        obs = env.reset()
        assert _np(obs).tobytes() == _np(twin.reset()).tobytes()
        for it in range(5):
            token = env.save_state()
            for c, cand in enumerate(cands):
                back = env.restore_state(token)
                assert _np(back).tobytes() == _np(obs).tobytes() and _np(back).shape == _np(obs).shape, (it, c)
                for k in range(4):
                    env.step(give(cand[4 * it + k]))
            env.restore_state(token)
            for k in range(3):
                got, want = env.step(give(acts[3 * it + k])), twin.step(give(acts[3 * it + k]))
                _same_step(got, want, (it, k))
                obs = _np(got[0]).copy()
            token.close()
            token.close()
        if path == "drivers":  # a masked restore: environment 0 goes back, environment 1 goes on; host state follows the mask
            third = sga.VectorScenarioEnv(objs, **kw)
            third.reset()
            for k in range(15):
                third.step(acts[k])
            token = env.save_state()
            for k in range(2):
                env.step(cands[0][k])
                third.step(cands[0][k])
            env.restore_state(token, mask=np.array([True, False]))
            got, back, on = env.step(acts[20]), twin.step(acts[20]), third.step(acts[20])
            drv = np.array([0, 0, 1, 1])
            for i, ref in ((0, back), (1, on)):
                assert got[1][i] == ref[1][i] and got[2][i] == ref[2][i]
                assert _np(got[0])[drv == i].tobytes() == _np(ref[0])[drv == i].tobytes(), i
                for key in ("driver_reward", "driver_progress", "driver_route", "driver_flags"):
                    assert _np(got[3][key])[drv == i].tobytes() == _np(ref[3][key])[drv == i].tobytes(), (i, key)
            third.close()
    finally:
        env.close()
        twin.close()


# -------------------------------------------------------------------------------------------------------- 9. lifecycle and refusals
@gpu
def test_lifecycle_and_refusals(sga):  # noqa: F811
    INVALID, STATE = -1, -3
    cfg = TE.column_batch()
    eng = sga.RolloutEngine(len(cfg["scs"]), PS.COLUMN_E, timestep=PS.DT, terminal_conditions=TE.TERMS, event_capacity=16)
    other = TE._engine(sga, cfg)
    lib, h = eng.lib, eng.h
    s, n = C.c_void_p(), C.c_uint64()
    msg = lambda: lib.sg_last_error(h).decode()  # noqa: E731
    assert lib.sg_snapshot_create(None, C.byref(s)) == INVALID and lib.sg_snapshot_create(h, None) == INVALID
    assert lib.sg_snapshot_create(h, C.byref(s)) == STATE and "no scenarios uploaded" in msg() and not s.value  # before sg_upload
    eng.upload(PS.pack(cfg["scs"]))
    TE._arm(eng, cfg)
    eng.step_drivers_policy(None, 3)
    assert lib.sg_snapshot_create(h, C.byref(s)) == 0 and s.value
    foreign = other.snapshot()
    before = _snapshot(eng)
    # NULL arguments, a snapshot of another handle
    for fn in (lib.sg_snapshot_save, lib.sg_snapshot_restore):
        assert fn(None, s, None, 0) == INVALID and fn(h, None, None, 0) == INVALID
        assert fn(h, foreign._s, None, 0) == INVALID and "another handle" in msg()
    assert lib.sg_snapshot_bytes(h, None, C.byref(n)) == INVALID and lib.sg_snapshot_bytes(h, s, None) == INVALID
    assert lib.sg_snapshot_bytes(h, foreign._s, C.byref(n)) == INVALID and lib.sg_snapshot_destroy(h, foreign._s) == INVALID
    assert lib.sg_snapshot_destroy(h, None) == INVALID and lib.sg_snapshot_destroy(None, s) == INVALID
    _assert_same(_snapshot(eng), before, "after the refused calls")
    assert lib.sg_snapshot_bytes(h, s, C.byref(n)) == 0 and n.value > 0
    # an sg_set_rss toggle, and back
    eng.set_rss(True)
    for fn in (lib.sg_snapshot_save, lib.sg_snapshot_restore):
        assert fn(h, s, None, 0) == STATE and "sg_set_rss" in msg()
    eng.set_rss(False)
    _assert_same(_snapshot(eng), before, "after the calls refused for sg_set_rss")
    assert lib.sg_snapshot_restore(h, s, None, 0) == 0
    # sg_set_drivers: the same list again is a change all the same (the accounting rows are per position in the list)
    eng.set_drivers(cfg["scen"], cfg["slot"])
    TE._arm(eng, cfg)
    before = _snapshot(eng)
    for fn in (lib.sg_snapshot_save, lib.sg_snapshot_restore):
        assert fn(h, s, None, 0) == STATE and "sg_set_drivers" in msg()
    _assert_same(_snapshot(eng), before, "after the calls refused for sg_set_drivers")
    assert lib.sg_snapshot_destroy(h, s) == 0
    # sg_upload
    assert lib.sg_snapshot_create(h, C.byref(s)) == 0
    eng.upload(PS.pack(cfg["scs"]))
    before = _snapshot(eng)
    for fn in (lib.sg_snapshot_save, lib.sg_snapshot_restore):
        assert fn(h, s, None, 0) == STATE and "sg_upload" in msg()
    _assert_same(_snapshot(eng), before, "after the calls refused for sg_upload")
    assert lib.sg_snapshot_bytes(h, s, C.byref(n)) == 0 and lib.sg_snapshot_destroy(h, s) == 0
    assert lib.sg_snapshot_destroy(h, s) == INVALID  # (gone)
    # create / destroy in a loop: the size stays; close() twice; a closed snapshot raises; close() of the engine frees the rest
    sizes = []
    for _ in range(4):
        snap = eng.snapshot()
        sizes.append(snap.nbytes)
        snap.close()
        snap.close()
    assert len(set(sizes)) == 1 and sizes[0] > 0
    with pytest.raises(RuntimeError, match="closed"):
        snap.restore()
    left = [eng.snapshot() for _ in range(3)]
    eng.close()
    for snap in left:
        snap.close()
    foreign.close()
    other.close()


@gpu
def test_refused_after_a_queue_give_up(sga, monkeypatch):  # noqa: F811
    """A persistent launch that gave up (on demand, as in test_queue_give_up_is_loud_and_sticky: a limit of one microsecond) leaves
    the state undefined: create, save and restore say so, with its message, until sg_reset starts the batch anew."""
    import scenario_gym_amd._lib as L
    from scenario_gym_amd import synthetic

    R, E, steps = 1024, 64, 400
    packed = synthetic.make_batch(R, E, n_steps=steps, ego_kind=L.KIND_AGENT_PID, extent=30.0)
    eng = sga.RolloutEngine(R, E, timestep=DT, terminal_conditions=["max_length"], event_capacity=64)
    eng.upload(packed)
    snap = eng.snapshot()
    start = _snapshot(eng)
    monkeypatch.setenv("SG_QUEUE_TIMEOUT_US", "1")
    eng.rollout_async(steps, do_reset=True)
    with pytest.raises(RuntimeError, match="gave up"):
        eng.synchronize()
    for call in (snap.save, snap.restore, eng.snapshot):
        with pytest.raises(RuntimeError, match="gave up"):
            call()
    monkeypatch.delenv("SG_QUEUE_TIMEOUT_US")
    eng.reset()
    eng.step(3)
    snap.restore()
    _assert_same(_snapshot(eng), start, "the snapshot of before the give-up")
    eng.close()
