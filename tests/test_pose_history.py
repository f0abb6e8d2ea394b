"""Pose-history observations (sg_pose_history, sg_pose_history_observers): where the ego of every scenario, or any observer of
sg_set_observers, and the k entities nearest to it were at the last n_samples rows of the pose record, in the observer's current
frame.  The reference has no such sensor, so the yardstick is history_scenes.history_reference -- the definition in include/sgym.h
restated in numpy over the record read back with RolloutEngine.record, the raw state view and the oracle's sin / cos.  Every
comparison is bit for bit on the features and exact on slots and counts.
"""
import os
import re
import types

import numpy as np
import pytest

import history_scenes as HS

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sg_pose_history", "sg_pose_history_observers")
SG_ERR_INVALID, SG_ERR_STATE = -1, -3
INF = float("inf")


@pytest.fixture
def sga():
    import scenario_gym_amd as sga

    return sga


# ---------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_the_history_calls():
    """include/sgym.h declares both calls with the agreed signature and limits, _lib.SYMBOLS names them, and the ABI version is
    still 7 (a purely additive change)."""
    import scenario_gym_amd._lib as L

    header = open(os.path.join(ROOT, "include", "sgym.h")).read()
    assert L.ABI_VERSION == 7 and re.search(r"#define SG_ABI_VERSION 7\b", header)
    assert re.search(r"#define SG_HIST_MAX_SAMPLES 64\b", header) and L.HIST_MAX_SAMPLES == 64
    assert re.search(r"#define SG_HIST_MAX_STRIDE \(1 << 20\)", header) and L.HIST_MAX_STRIDE == 1 << 20 and L.HIST_NFEAT == 6
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS
        assert re.search(r"\bint " + name + r"\(sg_handle \*h, int32_t n_samples, int32_t stride, int32_t k, double radius,\s*double \*feat,"
                         r"\s*int32_t \*slots,\s*int32_t \*count, int32_t outputs_device\);", header), name


def _record(tracks, dt=0.5):
    """A hand-made record of one scenario: tracks[e] = the (x, y, heading) of entity e row by row, None where it is absent.
    Returns (rec_t [rows, 1], rec [rows, 1, E, 6], state_at(n))."""
    rows, E = len(tracks[0]), len(tracks)
    rec_t, rec = (dt * np.arange(rows))[:, None], np.full((rows, 1, E, 6), np.nan)
    for e, track in enumerate(tracks):
        for n, p in enumerate(track):
            if p is not None:
                rec[n, 0, e] = (p[0], p[1], 0.0, p[2], 0.0, 0.0)
    return rec_t, rec, lambda n: HS.state_of_record(rec_t, rec, n)


def test_yardstick_on_hand_made_records(oracle):
    """The numpy restatement on records whose answers are worked out by hand."""
    # an observer driving +x at 2 m/s, heading 0, dt 0.5: a row is 1 m behind the next; stride 2 looks 2 m back per sample
    rows = 7
    me = [(1.0 * n, 0.0, 0.0) for n in range(rows)]
    late = [None, None, None] + [(1.0 * n, 3.0, 0.0) for n in range(3, rows)]            # spawns at row 3
    gap = [(1.0 * n + 1.0, -2.0, 0.0) if n != 4 else None for n in range(rows)]          # a NaN row between valid ones
    far = [(100.0, 0.0, 0.0)] * rows
    rec_t, rec, state_at = _record([me, late, gap, far])
    assert [oracle.sincos(0.0)] == [(0.0, 1.0)]
    feat, slots, count = HS.history_reference(oracle, rec_t, rec, state_at(6), 0, 0, 4, 2, 0, INF)
    assert feat.shape == (1, 4, 6) and slots.shape == (0,) and count == 3
    assert feat[0].tolist() == [[-2.0 * j, 0.0, 1.0, 0.0, 1.0 * j, 1.0] for j in range(4)]
    assert not np.signbit(feat[0, 0, 4])  # the age of sample 0 is +0.0
    # the same scene with the observer's heading at pi / 2: what lay behind now lies to its right, the old headings read as a
    # quarter turn clockwise
    turned = [(p[0], p[1], np.pi / 2) if n == 6 else p for n, p in enumerate(me)]
    rec_t2, rec2, state2 = _record([turned, late, gap, far])
    f2, _, _ = HS.history_reference(oracle, rec_t2, rec2, state2(6), 0, 0, 4, 2, 0, INF)
    want = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 1.0]] + [[0.0, 2.0 * j, 0.0, -1.0, 1.0 * j, 1.0] for j in range(1, 4)])
    assert np.abs(f2[0] - want).max() < 1e-15 and f2[0, 0].tolist() == want[0].tolist()
    # neighbours: by distance at the current state (row 6: gap at sqrt(5), late at 3, far at 94), their rows in the observer's frame
    feat, slots, count = HS.history_reference(oracle, rec_t, rec, state_at(6), 0, 0, 7, 1, 2, INF)
    assert slots.tolist() == [2, 1] and count == 3
    # ... the neighbour that spawned late: rows 6, 5, 4, 3 are valid, the three before its first are zeros
    assert feat[2, :, 5].tolist() == [1, 1, 1, 1, 0, 0, 0] and feat[2, :4, 0].tolist() == [0.0, -1.0, -2.0, -3.0] and (feat[2, :4, 1] == 3.0).all()
    assert not feat[2, 4:].any() and not np.signbit(feat[2, 4:]).any()
    # ... the neighbour with a NaN row between two valid ones: sample 2 (row 4) alone is invalid
    assert feat[1, :, 5].tolist() == [1, 1, 0, 1, 1, 1, 1] and feat[1, :, 0].tolist() == [1.0, 0.0, 0.0, -2.0, -3.0, -4.0, -5.0]
    assert feat[1, :, 4].tolist() == [0.0, 0.5, 0.0, 1.5, 2.0, 2.5, 3.0]
    # n_samples * stride larger than L: the samples before the episode began are zeros
    feat, _, _ = HS.history_reference(oracle, rec_t, rec, state_at(2), 0, 0, 5, 1, 0, INF)
    assert feat[0, :, 5].tolist() == [1, 1, 1, 0, 0] and feat[0, :3, 0].tolist() == [0.0, -1.0, -2.0] and not feat[0, 3:].any()
    feat, _, _ = HS.history_reference(oracle, rec_t, rec, state_at(6), 0, 0, 3, 40, 0, INF)
    assert feat[0, :, 5].tolist() == [1, 0, 0]
    # k larger than the number of candidates, and a radius that cuts the list: zero rows behind the last neighbour
    feat, slots, count = HS.history_reference(oracle, rec_t, rec, state_at(6), 0, 0, 2, 1, 5, INF)
    assert slots.tolist() == [2, 1, 3, -1, -1] and count == 3 and not feat[4:].any() and feat[3, :, 5].all()
    feat, slots, count = HS.history_reference(oracle, rec_t, rec, state_at(6), 0, 0, 2, 1, 2, 3.0)
    assert slots.tolist() == [2, 1] and count == 2
    feat, slots, count = HS.history_reference(oracle, rec_t, rec, state_at(6), 0, 0, 2, 1, 2, 2.5)
    assert slots.tolist() == [2, -1] and count == 1 and not feat[2].any()
    # an absent observer (the late spawner before it spawns): count -1, no neighbours, zeros
    feat, slots, count = HS.history_reference(oracle, rec_t, rec, state_at(2), 0, 1, 3, 1, 2, INF)
    assert count == -1 and slots.tolist() == [-1, -1] and not feat.any() and not np.signbit(feat).any()
    # a stale record: rec_rows stayed behind n_steps + 1
    st = state_at(6)
    st["n_steps"] = st["n_steps"] + 2
    feat, slots, count = HS.history_reference(oracle, rec_t, rec, st, 0, 0, 3, 1, 2, INF)
    assert count == -2 and slots.tolist() == [-1, -1] and not feat.any() and not np.signbit(feat).any()


def test_python_refusals_that_need_no_device(sga):
    """driver_history without drivers, driver_history without max_length, a malformed dict; the sensor without record=True."""
    from scenario_gym_amd.state import State

    with pytest.raises(ValueError, match="driver_history: needs a driver list"):
        sga.VectorScenarioEnv([], driver_history=dict(samples=4))
    with pytest.raises(ValueError, match="max_length"):
        sga.VectorScenarioEnv([], drivers=[], terminal_conditions=["ego_collision"], driver_history=dict(samples=4))
    with pytest.raises(ValueError, match="samples"):
        sga.VectorScenarioEnv([], drivers=[], driver_history=dict(stride=2))
    gym = sga.BatchedScenarioGym(record=False)
    entity = object()
    state = State.__new__(State)
    state._gym, state._i, state._scenario = gym, 0, types.SimpleNamespace(ego=entity, entities=[entity])
    sensor = sga.PoseHistorySensor(entity, n_samples=4, stride=2, k=3, radius=9.0)
    assert sensor.output_shape == (4, 4, 6)
    with pytest.raises(RuntimeError, match=r"pose_history needs BatchedScenarioGym\(record=True\)"):
        sensor.step(state)
    with pytest.raises(RuntimeError, match=r"recorded_poses needs BatchedScenarioGym\(record=True\)"):  # (the wording it follows)
        gym._fetch_record()


@pytest.mark.parametrize("E", HS.WIDTHS)
def test_device_scenes_exercise_the_kernel(oracle, E):
    """The scenes of the GPU tests through the yardstick on a record made without a device (the oracle's rollout, overlaid with
    what the tests feed): the sweep of every width -- the states after reset and after every tick, every PARAMS row, its observer
    list -- holds a valid neighbour sample with j > 0, an invalid sample from before the episode, an invalid sample on a NaN row
    that lies between valid ones, a zero row behind the last neighbour, an absent observer, and a neighbour whose slot is >= 64.
    A condition on the inputs, not a tolerance.  The last one cannot hold for the three-entity scene, which has no slot 64: it is
    required of every width that has one."""
    rec_t, rec = HS.cpu_record(oracle, E)
    seen = HS.coverage(oracle, rec_t, rec, E, range(HS.STEPS + 1))
    for case, n in seen.items():
        assert n > 0 or (case == "neighbour_slot_64" and E <= 64), (case, seen)
    assert E <= 64 or seen["neighbour_slot_64"] >= 100
    assert {(H, s) for H, s, _, _ in HS.PARAMS} >= {(1, 1), (64, 1), (5, 3)} and {k for _, _, k, _ in HS.PARAMS} >= {0, 32}
    assert {r for _, _, _, r in HS.PARAMS} >= {0.0, INF, 6.0} and max(s for _, s, _, _ in HS.PARAMS) > HS.STEPS


# ---------------------------------------------------------------------------------------------------- GPU: the C ABI
def _cc(shape, dtype):
    """A host array whose every byte is 0xCC."""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xCC, np.uint8).view(dtype).reshape(shape)


def _untouched(*arrays):
    return all((a.view(np.uint8) == 0xCC).all() for a in arrays)


def _raw(eng, n, H, stride, k, radius, observers, want_slots=True, want_count=True):
    """One of the two calls through ctypes into 0xCC-filled host buffers of n observers: (rc, feat, slots, count)."""
    feat, slots, count = _cc((n, 1 + max(k, 0), max(H, 0), 6), np.float64), _cc((n, max(k, 0)), np.int32), _cc((n,), np.int32)
    call = eng.lib.sg_pose_history_observers if observers else eng.lib.sg_pose_history
    rc = call(eng.h, H, stride, k, radius, feat.ctypes.data, slots.ctypes.data if want_slots and slots.size else None,
              count.ctypes.data if want_count else None, 0)
    return rc, feat, slots, count


def _engine(sga, E, cap=HS.CAP, **kw):
    """(engine, fed) of the scene of width E with its observer list set, after the reset of the upload."""
    packed, fed = HS.batch(E)
    eng = sga.RolloutEngine(HS.n_scenarios(E), E, timestep=HS.DT, record_capacity=cap, **kw)
    eng.upload(packed)
    eng.set_observers(*HS.observers(E))
    return eng, fed


def _tick(eng, fed, n):
    eng.set_external_poses(fed[n])
    eng.step(1)


def _view(eng, cap=HS.CAP):
    """(rec_t, rec, raw state) of the engine as it is."""
    rec_t, rec = eng.record(cap)
    return rec_t, rec, eng.state(raw=True)


def _check_state(eng, oracle, E, params, tag, nearest=False):
    """Both calls on the engine's current state against the yardstick for every row of `params`; with `nearest`, also against
    sg_nearest_entities_observers on the same state.  Returns the bytes of everything the device wrote."""
    rec_t, rec, st = _view(eng)
    R = HS.n_scenarios(E)
    scen, slot = HS.observers(E)
    egos, zero = np.arange(R), np.zeros(R, np.int32)
    out = b""
    for H, stride, k, radius in params:
        rc, *got = _raw(eng, R, H, stride, k, radius, observers=False)
        assert rc == 0 and HS.same(got, HS.reference_rows(oracle, rec_t, rec, st, egos, zero, H, stride, k, radius)), (tag, "egos", H, stride, k, radius)
        rc, *seen = _raw(eng, len(scen), H, stride, k, radius, observers=True)
        want = HS.reference_rows(oracle, rec_t, rec, st, scen, slot, H, stride, k, radius)
        assert rc == 0 and HS.same(seen, want), (tag, "observers", H, stride, k, radius)
        out += b"".join(a.tobytes() for a in got + seen)
        # subject 0, sample 0 of a present observer is the observer itself, now: (0, 0, c*c + s*s, s*c - c*s, +0, 1) -- by the
        # yardstick's bits, whatever c*c + s*s rounds to
        here = want[2] >= 0
        assert (seen[0][here, 0, 0, :2] == 0).all() and (seen[0][here, 0, 0, 4:] == [0.0, 1.0]).all() and here.any()
        assert np.abs(seen[0][here, 0, 0, 2] - 1.0).max() < 1e-15 and np.abs(seen[0][here, 0, 0, 3]).max() < 1e-15
        if nearest and k > 0:
            nf, ns, nc = eng.nearest_entities_observers(k, radius)
            fresh = want[2] != -2
            assert seen[1][fresh].tobytes() == ns[fresh].tobytes() and seen[2][fresh].tobytes() == nc[fresh].tobytes()
            assert np.ascontiguousarray(seen[0][fresh][:, 1:, 0, 0:4]).tobytes() == np.ascontiguousarray(nf[fresh][..., 0:4]).tobytes()
    return out


@gpu
@pytest.mark.parametrize("E", HS.WIDTHS)
def test_device_matches_the_yardstick(sga, oracle, E):
    """The scene of every width -- one block shared with others, a second block (NB = 2), NB = 8, the wide path -- after reset
    (only sample 0 valid) and after each of STEPS single steps in which the blinkers come and go: the ego call and the observer
    call (duplicates, absent observers) equal the yardstick for every PARAMS row, slots, counts and the first four features of
    sample 0 equal sg_nearest_entities_observers, and a run that takes the same steps in one sg_step(n) leaves the same bytes."""
    eng, fed = _engine(sga, E)
    rec_t, rec, st = _view(eng)
    assert (st["rec_rows"] == 1).all() and not st["present"][HS.observers(E)].all()
    rc, feat, _, count = _raw(eng, HS.n_scenarios(E), 8, 1, 4, INF, observers=False)
    assert rc == 0 and (feat[count >= 0][:, 0, :, 5] == [1, 0, 0, 0, 0, 0, 0, 0]).all() and not feat[:, :, 1:].any()
    _check_state(eng, oracle, E, HS.PARAMS, "reset", nearest=True)
    for n in range(1, HS.STEPS + 1):
        _tick(eng, fed, n)
        _check_state(eng, oracle, E, HS.PARAMS if n in (1, 2, 5, 8, HS.STEPS) else HS.PARAMS[1:3], n, nearest=n in (2, HS.STEPS))
    assert (eng.state()["rec_rows"] == HS.STEPS + 1).all()
    # one multi-step call: the caller-run slots keep the pose fed last, so the twin that steps one at a time feeds once too
    eng.reset()
    twin, _ = _engine(sga, E)
    for e in (eng, twin):
        e.set_external_poses(fed[1])
    eng.step(6)
    for _ in range(6):
        twin.step(1)
    a = _check_state(eng, oracle, E, HS.PARAMS, "sg_step(6)")
    b = _check_state(twin, oracle, E, HS.PARAMS, "6 x sg_step(1)")
    assert a == b
    eng.close()
    twin.close()


@gpu
@pytest.mark.parametrize("E", [70, 520])
def test_reset_of_one_scenario_starts_its_history_anew(sga, oracle, E):
    """sg_reset_scenarios on scenario 1 in the middle of a run: its observers' histories have one valid sample, the other
    scenarios' rows keep their bytes; two ticks later the new episode has three."""
    eng, fed = _engine(sga, E)
    for n in range(1, 6):
        _tick(eng, fed, n)
    scen, slot = HS.observers(E)
    H, stride, k, radius = 8, 1, 4, INF
    rc, *before = _raw(eng, len(scen), H, stride, k, radius, observers=True)
    mask = np.zeros(HS.n_scenarios(E), np.uint8)
    mask[1] = 1
    eng.reset_scenarios(mask)
    rc2, *after = _raw(eng, len(scen), H, stride, k, radius, observers=True)
    assert rc == 0 and rc2 == 0
    st = eng.state()
    assert st["rec_rows"].tolist() == [6, 1] + [6] * (HS.n_scenarios(E) - 2)
    hit = scen == 1
    assert hit.any() and all(a[~hit].tobytes() == b[~hit].tobytes() for a, b in zip(before, after))
    there = after[2] >= 0
    assert (after[0][hit & there][:, 0, :, 5] == [1] + [0] * (H - 1)).all() and not after[0][hit][:, :, 1:].any() and (hit & there).any()
    _check_state(eng, oracle, E, HS.PARAMS, "after the reset of scenario 1")
    for n in (6, 7):
        _tick(eng, fed, n)
    _check_state(eng, oracle, E, HS.PARAMS, "two ticks into the new episode")
    rc, feat, _, count = _raw(eng, HS.n_scenarios(E), H, stride, 0, radius, observers=False)
    assert rc == 0 and feat[1, 0, :, 5].tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and feat[0, 0, :, 5].all()
    eng.close()


@gpu
@pytest.mark.parametrize("how", ["tick_drivers", "step_drivers"])
def test_driver_episodes(sga, oracle, how):
    """The scene of width 70 with slot 2 of every scenario a driver and scenario 0 cut to 0.35 s.  sg_tick_drivers with auto-reset:
    scenario 0 reaches max_length and restarts within the run, and no sample of the finished episode appears afterwards -- the
    ego's valid samples are min(n_samples, rec_rows) at every tick, and every tick equals the yardstick.  sg_step_drivers: the
    same comparison with the steps the driver kernels take."""
    E = 70
    packed, fed = HS.batch(E)
    R = HS.n_scenarios(E)
    packed.length[0] = packed.t0[0] + 0.35
    eng = sga.RolloutEngine(R, E, timestep=HS.DT, record_capacity=HS.CAP, terminal_conditions=["max_length"])
    eng.upload(packed)
    eng.set_external_poses(fed[1])  # (the blinkers stay where they were put: they are no drivers)
    eng.set_drivers(np.arange(R), np.full(R, HS.driver_slot(E)))
    eng.set_observers(*HS.observers(E))
    acts = np.stack([np.linspace(0.5, 2.0, R), np.linspace(-0.1, 0.1, R)], -1)
    restarts = 0
    for n in range(1, 11):
        if how == "tick_drivers":
            eng.tick_drivers(acts, auto_reset=True)
        else:
            eng.step_drivers(acts[None], 1)
        st = eng.state()
        restarts += int(st["rec_rows"][0] == 1)
        assert (st["rec_rows"] == st["n_steps"] + 1).all()
        _check_state(eng, oracle, E, HS.PARAMS[1:4], (how, n))
        rc, feat, _, count = _raw(eng, R, 12, 1, 0, INF, observers=False)
        assert rc == 0 and (count >= 0).all()
        assert feat[:, 0, :, 5].sum(axis=1).tolist() == np.minimum(12, st["rec_rows"]).tolist(), n
    if how == "tick_drivers":
        assert restarts >= 2 and st["rec_rows"][1] == 11
    else:
        assert restarts == 0 and (st["rec_rows"] == 11).all()
    eng.close()


@gpu
def test_a_stale_record_is_refused_row_by_row(sga, oracle):
    """record_capacity = 4 and six steps: the record stopped at row 3 while the scenarios went on, so every observer of every
    scenario gets count -2, slots -1 and zero rows -- old rows are never presented as recent ones.  Up to the third step the record
    is full but current, and the answers are the yardstick's."""
    E = 70
    eng, fed = _engine(sga, E, cap=4)
    scen, slot = HS.observers(E)
    for n in range(1, 7):
        _tick(eng, fed, n)
        st = eng.state()
        rc, feat, slots, count = _raw(eng, len(scen), 4, 1, 3, INF, observers=True)
        assert rc == 0
        if n <= 3:
            assert (st["rec_rows"] == n + 1).all()
            rec_t, rec = eng.record(4)
            assert HS.same((feat, slots, count), HS.reference_rows(oracle, rec_t, rec, eng.state(raw=True), scen, slot, 4, 1, 3, INF)) and (count >= 0).any()
        else:
            assert (st["rec_rows"] == 4).all() and (st["n_steps"] == n).all()
            assert (count == -2).all() and (slots == -1).all() and not feat.any() and not np.signbit(feat).any()
            rc, feat, slots, count = _raw(eng, HS.n_scenarios(E), 2, 1, 0, INF, observers=False)
            assert rc == 0 and (count == -2).all() and not feat.any()
    eng.reset()  # a reset makes the record current again
    rc, feat, slots, count = _raw(eng, HS.n_scenarios(E), 2, 1, 0, INF, observers=False)
    assert rc == 0 and (count >= 0).all() and feat[:, 0, 0, 5].all()
    eng.close()


@gpu
def test_snapshot_restores_the_history(sga, oracle):
    """Save at step 5 and keep that history; three more steps; restore: the history has the kept bytes."""
    E = 70
    eng, fed = _engine(sga, E)
    for n in range(1, 6):
        _tick(eng, fed, n)
    snap = eng.snapshot()
    kept = _check_state(eng, oracle, E, HS.PARAMS, "at the save")
    for n in range(6, 9):
        _tick(eng, fed, n)
    assert _check_state(eng, oracle, E, HS.PARAMS, "three steps on") != kept
    snap.restore()
    assert _check_state(eng, oracle, E, HS.PARAMS, "restored") == kept
    snap.close()
    eng.close()


@gpu
@pytest.mark.parametrize("E", [3, 520])
def test_outputs_and_refusals(sga, oracle, E):
    """HOST and DEVICE outputs carry the same bytes, device outputs queued behind a step see that step, optional outputs may be
    NULL, 0xCC-filled outputs are fully overwritten (the comparisons above are over whole buffers); every refusal of the header
    is refused with its code and writes nothing."""
    import torch

    packed, fed = HS.batch(E)
    R = HS.n_scenarios(E)
    scen, slot = HS.observers(E)
    n = len(scen)
    # before the upload, and without a record
    eng = sga.RolloutEngine(R, E, timestep=HS.DT, record_capacity=HS.CAP)
    rc, *bufs = _raw(eng, R, 4, 1, 2, INF, observers=False)
    assert rc == SG_ERR_STATE and _untouched(*bufs)
    eng.upload(packed)
    bare = sga.RolloutEngine(R, E, timestep=HS.DT)
    bare.upload(packed)
    bare.set_observers(scen, slot)
    for observers in (False, True):
        rc, *bufs = _raw(bare, n, 4, 1, 2, INF, observers=observers)
        assert rc == SG_ERR_STATE and _untouched(*bufs) and b"pose record" in bare.lib.sg_last_error(bare.h)
    bare.close()
    # no observer list: SG_OK, nothing written
    rc, *bufs = _raw(eng, n, 4, 1, 2, INF, observers=True)
    assert rc == 0 and _untouched(*bufs)
    eng.set_observers(scen, slot)
    for m in range(1, 4):
        _tick(eng, fed, m)
    for observers in (False, True):
        for H, stride, k, radius in ((0, 1, 2, INF), (65, 1, 2, INF), (4, 0, 2, INF), (4, (1 << 20) + 1, 2, INF), (4, 1, -1, INF), (4, 1, 33, INF),
                                     (4, 1, 2, -1.0), (4, 1, 2, float("nan"))):
            rc, *bufs = _raw(eng, n, H, stride, k, radius, observers=observers)
            assert rc == SG_ERR_INVALID and _untouched(*bufs), (H, stride, k, radius)
        call = eng.lib.sg_pose_history_observers if observers else eng.lib.sg_pose_history
        slots, count = _cc((n, 2), np.int32), _cc((n,), np.int32)
        assert call(eng.h, 4, 1, 2, INF, None, slots.ctypes.data, count.ctypes.data, 0) == SG_ERR_INVALID and _untouched(slots, count)
    # the limits themselves are accepted; the optional outputs may be NULL
    rec_t, rec, st = _view(eng)
    rc, feat, _, _ = _raw(eng, n, 64, 1 << 20, 32, INF, observers=True, want_slots=False, want_count=False)
    assert rc == 0 and feat.tobytes() == HS.reference_rows(oracle, rec_t, rec, st, scen, slot, 64, 1 << 20, 32, INF)[0].tobytes()
    # DEVICE outputs, queued behind a step, not waited for by the call: the bytes of the HOST call on the stepped state
    H, stride, k, radius = 6, 2, 5, INF
    dev = [torch.full(shape, 0xCC, dtype=torch.uint8, device="cuda:0") for shape in ((n * (1 + k) * H * 6 * 8,), (n * k * 4,), (n * 4,))]
    torch.cuda.synchronize()
    _tick(eng, fed, 4)
    rc = eng.lib.sg_pose_history_observers(eng.h, H, stride, k, radius, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 1)
    assert rc == 0
    assert eng.lib.sg_synchronize(eng.h) == 0
    rc, *host = _raw(eng, n, H, stride, k, radius, observers=True)
    rec_t, rec, st = _view(eng)
    assert rc == 0 and (st["n_steps"] == 4).all() and HS.same(host, HS.reference_rows(oracle, rec_t, rec, st, scen, slot, H, stride, k, radius))
    assert all(d.cpu().numpy().tobytes() == h.tobytes() for d, h in zip(dev, host))
    # the Python wrappers: shapes, and the bytes of the raw calls
    got = eng.pose_history_observers(H, stride, k, radius)
    assert HS.same(got, host) and got[0].shape == (n, 1 + k, H, 6)
    on_dev = eng.pose_history_observers(H, stride, k, radius, torch_out=True)
    assert all(t.is_cuda for t in on_dev) and HS.same([t.cpu().numpy() for t in on_dev], host)
    own = eng.pose_history(3)
    assert own[0].shape == (R, 1, 3, 6) and own[1].shape == (R, 0) and own[0].tobytes() == _raw(eng, R, 3, 1, 0, INF, observers=False)[1].tobytes()
    eng.close()


# ---------------------------------------------------------------------------------------------------- GPU: the Python layers
def _scenario_objects(scs):
    from test_host_api import scenario_from_arrays

    return [scenario_from_arrays(sc, ["ego" if i == sc["ego"] else f"entity_{i}" for i in range(len(sc["etype"]))]) for sc in scs]


@gpu
@pytest.mark.parametrize("device_tick", [False, True])
def test_vector_env_driver_history(sga, device_tick):
    """VectorScenarioEnv(drivers=..., driver_history=dict(samples=6, stride=2, k=3, radius=40)) on the column scene, scenario 0 cut
    at 1.25 s so that it restarts within the run, with and without device_tick: reset() and every step() report the rows of
    engine.pose_history_observers called by hand on the state behind the auto-reset, count is never -2, and a restarted
    environment starts with one valid sample.  A caller's own observer list is swapped around the call and put back."""
    import policy_scenes as PS
    import torch

    cfg = PS.column(2, mixed=True)
    cfg["scs"][0] = PS.cut_at(cfg["scs"][0], 1.25)
    objs = _scenario_objects(cfg["scs"])
    drivers = [[5, 6], [5, 6]]
    H, stride, k, radius = 6, 2, 3, 40.0
    kw = dict(timestep=PS.DT, n=8, terminal_conditions=["max_length"], max_steer=0.7, max_accel=5.0, drivers=drivers, torch_obs=device_tick,
              device_tick=device_tick, driver_history=dict(samples=H, stride=stride, k=k, radius=radius))
    env = sga.VectorScenarioEnv(objs, **kw)
    from scenario_gym_amd.packing import pack_scenarios

    packed, _ = pack_scenarios(objs, lambda scenario, entity: None)
    longest = float(np.max(packed.length - packed.t0))  # max_length ends an episode behind step floor(longest / dt): + slack + the reset row
    assert longest > 5.0 and env.engine.cfg.record_capacity == int(np.floor(longest / PS.DT)) + 2
    env.set_observers([[1], [2, 3]])  # (not the drivers: the environment swaps the lists around its call)

    def by_hand():
        env.engine.set_observers(env._drv_env, env._drv_slot)
        out = env.engine.pose_history_observers(H, stride, k, radius)
        env.engine.set_observers(env._obs_env, env._obs_slot)
        return out

    def host(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else x

    def reported(info):
        return [host(info[key]) for key in ("driver_history", "driver_history_slots", "driver_history_count")]

    env.reset()
    first = reported(env.reset_info)
    assert HS.same(first, by_hand()) and first[0].shape == (4, 1 + k, H, 6) and (first[0][:, 0, :, 5] == [1, 0, 0, 0, 0, 0]).all()
    acts = np.ascontiguousarray(PS.caller_actions(4, [], seed=11))
    acts[..., 0] += 1.0
    restarted, fresh = np.zeros(2, bool), 0
    for n in range(30):
        a = torch.as_tensor(acts[n], device="cuda:0") if device_tick else acts[n]
        obs, reward, done, info = env.step(a)
        got = reported(info)
        if device_tick:
            assert all(info[key].is_cuda for key in ("driver_history", "driver_history_slots", "driver_history_count"))
        assert HS.same(got, by_hand()), n
        assert (got[2] >= 0).all(), "count -2: the record does not cover the episode"
        done = host(done)
        restarted |= done
        for d in np.nonzero(done[env._drv_env])[0]:
            fresh += 1
            assert got[0][d, 0, :, 5].tolist() == [1, 0, 0, 0, 0, 0] and not got[0][d, :, 1:].any()
        assert env.engine._n_obs == 3 and np.array_equal(env._obs_env, [0, 1, 1])  # (the caller's list is back in place)
    assert restarted[0] and not restarted[1] and fresh >= 2
    assert got[0][2, 0, :, 5].all() and got[0][2, 1, :, 5].any()  # environment 1: a full history, and a neighbour's
    own = env.pose_history(4, 1, 2, 30.0)
    assert tuple(own[0].shape) == (2, 3, 4, 6) and HS.same([host(t) for t in own], env.engine.pose_history(4, 1, 2, 30.0))
    env.close()


@gpu
def test_sensor_on_the_ego_and_on_another_entity(sga, oracle):
    """PoseHistorySensor on the ego, on a non-ego entity inside a CombinedSensor and stepped by the caller, in a
    BatchedScenarioGym(record=True) batch: the observation equals state.recorded_poses() put back into a record and transformed by
    the yardstick."""
    from test_nearest import _scenarios

    scs, _ = _scenarios(sga, 2, 12, 30, seed=5, ego_at=4)
    gym = sga.BatchedScenarioGym(timestep=0.1, record=True)
    gym.set_scenarios(scs)
    for _ in range(6):
        gym.step()
    for i, state in enumerate(gym.states):
        ents = state.scenario.entities
        here = [e for e in ents if e in state.poses and e is not state.scenario.ego]
        assert state.scenario.ego is ents[4] and len(here) >= 3
        rows = 7
        rec_t, rec = np.zeros((rows, 1)), np.full((rows, 1, len(ents), 6), np.nan)
        rec_t[:, 0] = state.recorded_poses(state.scenario.ego)[:, 0]
        for j, e in enumerate(ents):
            for row in state.recorded_poses(e):
                rec[int(np.nonzero(rec_t[:, 0] == row[0])[0][0]), 0, j] = row[1:]
        st = HS.state_of_record(rec_t, rec, rows - 1)
        for entity, sensor in ((ents[4], sga.PoseHistorySensor(ents[4], 5, 2, 3, 25.0)),
                               (here[0], sga.CombinedSensor(here[0], sga.PoseHistorySensor(here[0], 4, 1, 2), sga.NearestEntitiesSensor(here[0], k=2)))):
            obs = sensor.reset(state)
            leaf = sensor.sensors[0] if isinstance(sensor, sga.CombinedSensor) else sensor
            feat, slots, count = HS.history_reference(oracle, rec_t, rec, st, 0, ents.index(entity), leaf.n_samples, leaf.stride, leaf.k, leaf.radius)
            assert obs.history.tobytes() == feat[0].tobytes() and obs.neighbour_histories.tobytes() == feat[1:].tobytes() and obs.entity is entity
            assert obs.history_neighbours == [ents[q] for q in slots if q >= 0] and len(obs.history_neighbours) >= 2 and obs.history[:, 5].sum() >= 3
            if leaf is not sensor:
                assert obs.neighbours == obs.history_neighbours == state.nearest_entities(2, entity=entity)[0] and obs.features.shape == (2, 8)
            else:
                assert isinstance(obs, sga.PoseHistoryObservation)
    gym.close()
