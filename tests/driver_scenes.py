"""Scenes for the driver tests (tests/test_drivers.py, tests/golden/make_golden_drivers.py): small batches whose policy-driven
vehicles are placed so that they do what the tests are about.

Every scenario has the same skeleton, far from the background traffic (x around -200):
  role "a"   starts at (-200, 0) heading 0 at 6 m/s, towards ...
  the victim a static entity at (-191, 0.3) (slot VICTIM, never one of the straddling driver slots), which "a" reaches after
             about 0.8 s, and ...
  role "b"   which starts at (-178, 0) heading pi at 6 m/s: head-on with "a" from about 1.3 s on
  role "c"   whose trajectory starts at t = 1.0 (the scenario starts at 0): it spawns late, with controller speed 0
  others     constant-speed straight lines on a 14 m grid at x >= 0, some static, some present for a part of the time only
The action sequences are calm for the first CALM steps (small steering: the skeleton's collisions happen) and wild afterwards
(beyond max_steer / max_accel), each driver with its own bias, so every driver leaves its recorded trajectory by metres.
"""
import numpy as np

DT, STEPS, R = 0.1, 40, 6
LENGTH = 4.0
CALM = 15
VICTIM = 1
CAR = (2.0, 4.2, 1.37, 0.0)  # width, length, center_x, center_y
KIND_NONE, KIND_REPLAY, KIND_AGENT_REPLAY, KIND_AGENT_VEHICLE, KIND_AGENT_EXTERNAL = 0, 1, 2, 4, 6
NCTRL = 16
DEFAULT_CTRL = np.array([0.7, 5.0, np.nan, 0.0, 0.03054, 1.5709, 0.3753, 1.8970, 0.0204, 0.0, 5.0, 0.0, 1.0, 0, 0, 0])


def _line(t0, t1, x, y, h, v):
    """Two knots of a straight constant-speed line (one knot when t0 == t1: a static entity)."""
    ts = np.array([t0]) if t0 == t1 else np.array([t0, t1])
    k = np.zeros((len(ts), 7))
    k[:, 0] = ts
    k[:, 1] = x + v * np.cos(h) * (ts - t0)
    k[:, 2] = y + v * np.sin(h) * (ts - t0)
    k[:, 4] = h
    return k


def scenario(E, drivers, ego, rng):
    """One scenario of E entities as plain arrays.  drivers: [(slot, role)], role in "a", "b", "c", "free"."""
    role = dict(drivers)
    knots = []
    for i in range(E):
        what = role.get(i)
        if what == "a":
            k = _line(0.0, LENGTH, -200.0, 0.0, 0.0, 6.0)
        elif what == "b":
            k = _line(0.0, LENGTH, -178.0, 0.0, np.pi, 6.0)
        elif what == "c":
            k = _line(1.0, LENGTH, -200.0, 40.0, 0.5 * np.pi, 4.0)
        elif i == VICTIM:
            k = _line(0.5, 0.5, -191.0, 0.3, 0.0, 0.0)
        else:
            x, y, h, v, u = (i % 26) * 14.0, (i // 26) * 14.0, rng.uniform(-np.pi, np.pi), rng.uniform(0.0, 3.0), rng.random()
            if what == "free":  # (a driver: always there, never at rest, so that its actions take it off its trajectory)
                k = _line(0.0, LENGTH, x, y, h, 1.0 + v / 1.5)
            elif i != ego and u < 0.15:
                k = _line(1.5, 1.5, x, y, h, 0.0)
            elif i != ego and u < 0.3:
                k = _line(0.45, 3.05, x, y, h, v)
            else:
                k = _line(0.0, LENGTH, x, y, h, v)
        knots.append(k)
    off = np.concatenate([[0], np.cumsum([len(k) for k in knots])]).astype(np.int64)
    ctrl = np.tile(DEFAULT_CTRL, (E, 1))
    for slot, _ in drivers:  # every driver its own controller row
        ctrl[slot, 0] = rng.uniform(0.3, 0.9)
        ctrl[slot, 1] = rng.uniform(2.0, 6.0)
        ctrl[slot, 2] = np.nan if rng.random() < 0.5 else rng.uniform(7.5, 9.0)
        ctrl[slot, 3] = float(rng.random() < 0.5 or slot == VICTIM)  # (the static victim as a driver: it can leave in either direction)
    kind = np.full(E, KIND_REPLAY, np.int32)
    kind[ego] = KIND_AGENT_REPLAY
    for slot, _ in drivers:
        kind[slot] = KIND_AGENT_EXTERNAL
    return dict(knot_off=off, knots=np.concatenate(knots), bbox=np.tile(np.array(CAR), (E, 1)), etype=np.zeros(E, np.int32), ego=int(ego),
                t0=0.0, length=LENGTH, kind=kind, ctrl=ctrl, drivers=[s for s, _ in drivers])


def batch(E, drivers, egos=None, seed=0):
    """R scenarios.  drivers[r]: [(slot, role)] of scenario r; egos[r]: its ego slot (default 0)."""
    rng = np.random.default_rng([20250131, E, seed])
    egos = [0] * len(drivers) if egos is None else egos
    return [scenario(E, d, e, rng) for d, e in zip(drivers, egos)]


def actions(n_drivers, seed=0):
    """[STEPS, n_drivers, 2] (accel, steer): calm, then wild; every driver its own bias, every step its own values."""
    rng = np.random.default_rng([20250131, 77, seed, n_drivers])
    bias = rng.choice([-3.0, 3.0], n_drivers) + rng.uniform(-0.5, 0.5, n_drivers)
    a = np.empty((STEPS, n_drivers, 2))
    a[..., 0] = bias + rng.uniform(-1.0, 1.0, (STEPS, n_drivers))
    a[..., 1] = rng.uniform(-0.03, 0.03, (STEPS, n_drivers))
    a[CALM:, :, 0] = bias + rng.uniform(-7.0, 7.0, (STEPS - CALM, n_drivers))  # (beyond every max_accel of scenario())
    a[CALM:, :, 1] = rng.uniform(-1.5, 1.5, (STEPS - CALM, n_drivers))         # (... and every max_steer)
    return a


def pack(scs):
    """The batch as scenario_gym_amd PackedScenarios (kinds and controller rows as scenario() made them)."""
    from scenario_gym_amd.packing import pack_arrays

    return pack_arrays(scs, kinds=[s["kind"] for s in scs], ctrls=[s["ctrl"] for s in scs])


def driver_list(scs):
    """(scenario [n], slot [n]) of every driver of the batch, scenario by scenario in the order given to scenario()."""
    scen = [r for r, s in enumerate(scs) for _ in s["drivers"]]
    slot = [k for s in scs for k in s["drivers"]]
    return np.array(scen, np.int32), np.array(slot, np.int32)


# ---- the configurations of test 2: D = 0, 1 and 3 drivers per scenario in one batch, on slots that straddle the 64-slot blocks ----
def mixed_config(E):
    if E == 65:
        t1, t2, t3, s1, s2 = (0, 63, 64), (64, 0, 63), (63, 64, 0), 63, 64
    else:  # 520: also 255, 256, 519
        t1, t2, t3, s1, s2 = (0, 63, 64), (255, 256, 519), (519, 63, 255), 256, 519
    tri = lambda t: [(t[0], "a"), (t[1], "b"), (t[2], "c")]  # noqa: E731
    return [tri(t1), [(s1, "a")], [], tri(t2), [(s2, "a")], tri(t3)]


def all_config(E=65):
    """Every entity a driver: the skeleton on slots 0, 63, 64, everybody else (the victim too) free."""
    rest = [(i, "free") for i in range(E) if i not in (0, 63, 64)]
    return [[(0, "a"), (63, "b"), (64, "c")] + rest for _ in range(R)]


def expected_poses(O, sc, acts):
    """What the drivers of scenario `sc` must do, from the oracle: driver j's poses are those of sgo_rollout on the scenario with j
    as its only vehicle agent (the other drivers replay their trajectories: VehicleController never looks at another entity),
    forced steps, j's actions acts[:, j].  Returns (poses [STEPS + 1, n_drivers, 6] with NaN where j is not in the scene,
    speed [STEPS + 1, n_drivers] the controller's speed after every step)."""
    nd = len(sc["drivers"])
    poses, speed = np.full((STEPS + 1, nd, 6), np.nan), np.zeros((STEPS + 1, nd))
    for j, slot in enumerate(sc["drivers"]):
        kind = np.where(sc["kind"] == KIND_AGENT_EXTERNAL, KIND_REPLAY, sc["kind"]).astype(np.int32)
        kind[slot] = KIND_AGENT_VEHICLE
        o = O.rollout(sc["knot_off"], sc["knots"], sc["bbox"], sc["etype"], kind, sc["ego"], sc["t0"], sc["length"], DT, ctrl=sc["ctrl"],
                      actions=np.ascontiguousarray(acts[:, j]), max_steps=STEPS, force_steps=True)
        assert o["n_steps"] == STEPS
        poses[:, j], speed[:, j] = o["poses"][:, slot], o["extra"][:, slot, 0]
    return poses, speed
