"""The scenes of tests/test_pose_history.py and the yardstick they are judged by.

A scene is a seeded synthetic batch (scenario_gym_amd.synthetic) of R scenarios of E entities, 3 s long at DT = 0.1 s, in which
late spawners and early leavers are common (vanish_frac), with two kinds of slot changed to SG_KIND_AGENT_EXTERNAL:

  the blinkers  slot 1, and slot 66 where the scenario has one: the test feeds their poses tick by tick (`fed`), always within a few
                metres of where the ego starts, and feeds NaN -- the agent returned None -- at the ticks BLINKS: their record has NaN
                rows between valid ones, and the one at slot 66 is a near neighbour of the ego from the second block of 64 slots.
  the drivers   slot 2 of every scenario (where there is one): the slots sg_set_drivers lists in the episode tests.  In the runs that
                step with sg_step they are fed like a blinker that never blinks.

`history_reference` is the definition of sg_pose_history in include/sgym.h restated in numpy / plain Python floats (a * c + b * s
is two products and a sum: nothing fused) over the record read back with RolloutEngine.record, the raw state view and the oracle's
sincos.  `cpu_record` makes the record and the states of a scene without a device -- the oracle's rollout of the batch with the
caller-run slots replayed, overlaid with what the test feeds -- so that the scenes can be checked on the CPU for the cases the
kernel has to meet (`coverage`).
"""
import numpy as np

DT = 0.1
WIDTHS = (3, 70, 300, 520)   # one block shared; a second 64-block (NB = 2); NB = 8; the wide path
STEPS = 10                   # single steps of a run (the issue: at most 12)
BLINKS = (3, 4, 7)           # the ticks at which the blinkers return None
CAP = 16                     # record_capacity of the scene handles
KIND_REPLAY, KIND_AGENT_EXTERNAL = 1, 6
INF = float("inf")

# (n_samples, stride, k, radius) of the sweeps: k = 0 and 32, radius 0, finite and inf, n_samples 1 and 64, strides 1, 3 and one
# larger than the episode so far
PARAMS = ((1, 1, 0, INF), (4, 1, 3, INF), (64, 1, 32, INF), (5, 3, 8, 6.0), (6, 2, 32, 0.0), (3, 40, 2, INF), (8, 1, 5, 2.5))


def n_scenarios(E):
    return 4 if E <= 64 else 3


def blinkers(E):
    return [1] + ([66] if E > 66 else [])


def driver_slot(E):
    return 2 if E > 2 else None


def batch(E, seed=0):
    """(packed, fed [STEPS + 1, R, E, 6]): the batch with its caller-run slots marked, and the poses the test feeds ahead of tick
    n = 1 .. STEPS (row n; row 0 is unused; NaN everywhere but in the caller-run slots)."""
    from scenario_gym_amd import synthetic

    R = n_scenarios(E)
    packed = synthetic.make_batch(R, E, n_steps=30, timestep=DT, n_knots=16, extent=20.0, vanish_frac=0.4, seed=700 + E + seed)
    kind = packed.kind.reshape(R, E)
    fed = np.full((STEPS + 1, R, E, 6), np.nan)
    for r in range(R):
        x0, y0 = packed.knots[packed.knot_off[r * E], 1:3]  # where the ego starts
        for m, b in enumerate(blinkers(E)):
            kind[r, b] = KIND_AGENT_EXTERNAL
            for n in range(1, STEPS + 1):
                if n not in BLINKS:
                    fed[n, r, b] = (x0 + 1.5 + m + 0.25 * n, y0 + (1.0 if m else -1.25) + 0.125 * r, 0.0, 0.125 * n - 0.5 * m, 0.0, 0.0)
        d = driver_slot(E)
        if d is not None:
            kind[r, d] = KIND_AGENT_EXTERNAL
            for n in range(1, STEPS + 1):
                fed[n, r, d] = (x0 - 2.0 - 0.5 * n, y0 + 0.75, 0.0, 3.0 + 0.0625 * n, 0.0, 0.0)
    return packed, fed


def observers(E):
    """The observer list of a scene: every entity of scenario 0 (E <= 70) or a spread of it, the ego twice (a duplicate), the
    blinkers and picks of the other scenarios -- present or not, the tests assert that some are absent."""
    R = n_scenarios(E)
    first = np.arange(E) if E <= 70 else np.unique(np.concatenate([np.arange(0, E, 37), blinkers(E), [E - 1]]))
    rng = np.random.default_rng(E)
    scen = np.concatenate([np.zeros(len(first)), [0, 0], rng.integers(1, R, 12), np.repeat(np.arange(1, R), len(blinkers(E)))])
    slot = np.concatenate([first, [0, 0], rng.integers(0, E, 12), np.tile(blinkers(E), R - 1)])
    return scen.astype(np.int32), slot.astype(np.int32)


# ---------------------------------------------------------------------------------------------------- the yardstick
def select_nearest(poses, present, slot, k, radius):
    """The selection of sg_nearest_entities for a present observer `slot` of one scenario (poses [E, 6], present [E]): the slots of
    the at most k candidates by ascending (d2, slot), and the number of candidates."""
    with np.errstate(all="ignore"):
        dx, dy = poses[:, 0] - poses[slot, 0], poses[:, 1] - poses[slot, 1]
        d2 = dx * dx + dy * dy
        cand = present & (np.arange(len(present)) != slot) & np.isfinite(d2) & (d2 <= np.float64(radius) * np.float64(radius))
    idx = np.nonzero(cand)[0]
    return idx[np.lexsort((idx, d2[idx]))][:k], len(idx)


def history_reference(oracle, rec_t, rec, st, r, slot, n_samples, stride, k, radius):
    """The definition for observer `slot` of scenario r: rec_t [rows, R] and rec [rows, R, E, 6] the record, st the raw state view
    (poses, present, t, n_steps, rec_rows).  Returns (feat [1 + k, n_samples, 6], slots [k], count)."""
    feat, slots = np.zeros((1 + k, n_samples, 6)), np.full(k, -1, np.int32)
    L = int(st["rec_rows"][r])
    if L != int(st["n_steps"][r]) + 1:
        return feat, slots, -2
    if not st["present"][r, slot]:
        return feat, slots, -1
    xo, yo, ho = (float(v) for v in st["poses"][r, slot, [0, 1, 3]])
    s, c = oracle.sincos(ho)
    t = float(st["t"][r])
    near, count = select_nearest(st["poses"][r], st["present"][r], slot, k, radius)
    slots[:len(near)] = near
    for i, e in enumerate([slot] + [int(q) for q in near]):
        for j in range(n_samples):
            rho = L - 1 - j * stride
            if rho < 0:
                continue
            X, Y, Hd = (float(v) for v in rec[rho, r, e, [0, 1, 3]])
            if X != X:
                continue
            se, ce = oracle.sincos(Hd)
            dx, dy = X - xo, Y - yo
            feat[i, j] = (dx * c + dy * s, dy * c - dx * s, ce * c + se * s, se * c - ce * s, 0.0 if j == 0 else t - float(rec_t[rho, r]), 1.0)
    return feat, slots, count


def reference_rows(oracle, rec_t, rec, st, scen, slot, n_samples, stride, k, radius):
    """history_reference for the observers (scen[i], slot[i]): (feat [n, 1 + k, n_samples, 6], slots [n, k], count [n])."""
    out = [history_reference(oracle, rec_t, rec, st, int(r), int(e), n_samples, stride, k, radius) for r, e in zip(scen, slot)]
    n = len(out)
    return (np.array([o[0] for o in out]).reshape(n, 1 + k, n_samples, 6), np.array([o[1] for o in out], np.int32).reshape(n, k),
            np.array([o[2] for o in out], np.int32).reshape(n))


def same(got, want):
    """feat bit for bit, slots and count exactly."""
    return (got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes() and got[1].shape == want[1].shape
            and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]))


# ---------------------------------------------------------------------------------------------------- the scenes without a device
def cpu_record(oracle, E):
    """(rec_t [STEPS + 1, R], rec [STEPS + 1, R, E, 6]) of a scene as the device records it when the test steps it STEPS times and
    feeds `fed`: the oracle's rollout with the caller-run slots replayed, their rows from tick 1 on replaced by what was fed."""
    from scenario_gym_amd.packing import unpack_scenario

    packed, fed = batch(E)
    R = n_scenarios(E)
    rec_t, rec = np.zeros((STEPS + 1, R)), np.full((STEPS + 1, R, E, 6), np.nan)
    ext = packed.kind.reshape(R, E) == KIND_AGENT_EXTERNAL
    for r in range(R):
        s = unpack_scenario(packed, r)
        kind = np.where(np.asarray(s["kind"]) == KIND_AGENT_EXTERNAL, KIND_REPLAY, s["kind"]).astype(np.int32)
        o = oracle.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], kind, s["ego"], s["t0"], s["length"], DT, ctrl=s["ctrl"],
                           max_steps=STEPS, force_steps=True)
        assert o["n_steps"] == STEPS
        rec[:, r] = o["poses"][:STEPS + 1]
        rec_t[:, r] = s["t0"] + DT * np.arange(STEPS + 1)  # (the ages are not what the coverage is about)
        rec[1:, r, ext[r]] = fed[1:, r, ext[r]]
    return rec_t, rec


def state_of_record(rec_t, rec, n):
    """The raw state view after tick n of a run that recorded (rec_t, rec)."""
    R = rec.shape[1]
    return dict(poses=np.nan_to_num(rec[n]), present=~np.isnan(rec[n, :, :, 0]), t=rec_t[n], n_steps=np.full(R, n), rec_rows=np.full(R, n + 1))


def coverage(oracle, rec_t, rec, E, ticks):
    """Which of the cases the kernel has to meet occur when the sweep of a scene -- every PARAMS row for its observer list at the
    states after the ticks `ticks` -- goes through the yardstick: a dict of counts."""
    seen = dict(valid_neighbour_past=0, before_episode=0, nan_between_valid=0, row_behind_last=0, neighbour_slot_64=0, absent_observer=0)
    scen, slot = observers(E)
    for n in ticks:
        st = state_of_record(rec_t, rec, n)
        for H, stride, k, radius in PARAMS:
            feat, slots, count = reference_rows(oracle, rec_t, rec, st, scen, slot, H, stride, k, radius)
            valid = feat[..., 5] == 1.0
            seen["valid_neighbour_past"] += int(valid[:, 1:, 1:].sum())
            seen["absent_observer"] += int((count == -1).sum())
            seen["row_behind_last"] += int(((slots == -1) & (count >= 0)[:, None]).sum())
            seen["neighbour_slot_64"] += int((slots >= 64).sum())
            rho = n - np.arange(H) * stride
            seen["before_episode"] += int((count >= 0).sum()) * int((rho < 0).sum())
            for o in np.nonzero(count >= 0)[0]:
                for i, e in enumerate([slot[o]] + [q for q in slots[o] if q >= 0]):
                    v = valid[o, i]
                    for j in range(1, H - 1):  # an invalid sample inside the episode with valid ones on both sides: a NaN row
                        if rho[j] >= 0 and not v[j] and v[:j].any() and v[j + 1:].any():
                            seen["nan_between_valid"] += 1
    return seen
