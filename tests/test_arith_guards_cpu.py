"""The scenes of tests/arith_scenes.py do what they are for -- on the CPU, without a device.

  * yardstick: pair_terms (ped_pair with ExactArith, restated in Python floats with a once-rounded fma) implies, pair by pair
    in the oracle's order, the force the oracle reports -- bit for bit, signed zeros included -- on two-pedestrian scenes under
    default parameters, a head rotation, attraction on, sight weights off, and on every scene of every small family;
  * every family trips the guard it aims at, by at least the pairs it was built for (counts in the assertions), and the
    "just passes" twin of every threshold case trips nothing;
  * coverage cap: the only NaN rows of any scene are the ones its scene lists by name (the coincident pair, the pedestrian
    with the NaN coordinate): no scene drops out of the device comparison because the oracle gave up on it;
  * decisiveness: three wrong variants of the arithmetic, emulated in Python on the aimed operands, give other bits than IEEE.
"""
import math

import numpy as np
import pytest

import arith_scenes as A


def same_bits(a, b):
    """NaN positions equal and every other value equal as uint64: -0.0 != +0.0."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def implied_force(O, fam, o, k, i, sf, peds):
    """The social force on pedestrian i in the step from record row k, from pair_terms, neighbours in entity order."""
    c = 1 if fam.car else 0
    P, V = o["poses"][k], o["vels"][k]
    fx, fy = A.goal_force(P[i + c, 0], P[i + c, 1], peds[i, 2], peds[i, 3], peds[i, 4], V[i + c, 0], V[i + c, 1], sf)
    for j in range(len(peds)):
        if j != i and O.in_radius(P[i + c, 0], P[i + c, 1], A.RADIUS, P[j + c, 0], P[j + c, 1]):
            fx, fy = A.accumulate(fx, fy, A.terms_of(O, fam, o, k, i, j, sf), sf)
    return fx, fy


@pytest.fixture(scope="module")
def fams(oracle):
    return A.families(oracle)


@pytest.fixture(scope="module")
def runs(oracle, fams):
    """Every (family, parameter set, scene) through the oracle once: name -> list of (parameter-set name, sf, [oracle result per
    scene])."""
    out = {}
    for name, fam in fams.items():
        batch = A.pack(fam)
        out[name] = [(pn, sf, [A.run_oracle(oracle, fam, batch, r, sf) for r in range(len(fam.scenes))]) for pn, sf in fam.param_sets]
    return out


SMALL = [n for n in ("near", "negzero", "midpoint", "midpoint_sigma", "faint", "sliver", "insane", "params", "headrot_near",
                     "headrot_negzero", "headrot_midpoint", "headrot_car_near", "headrot_car_negzero", "headrot_car_midpoint")]


@pytest.fixture(scope="module")
def classes(oracle, fams, runs):
    """(family, parameter set, scene index, step, i, j) -> (guard set, terms) for every active pair of the small families."""
    out = {}
    for name in SMALL:
        fam = fams[name]
        for pn, sf, res in runs[name]:
            for r, o in enumerate(res):
                for k in range(o["n_steps"]):
                    for i, j in A.active_pairs(oracle, fam, o, k):
                        T = A.terms_of(oracle, fam, o, k, i, j, sf)
                        out[name, pn, r, k, i, j] = (A.guard_class(T, sf), T)
    return out


def test_exp_restatement_is_the_oracles(oracle):
    xs = [-1e-300, -5e-11, -0.3, -1.0, -2.0, -247.3, -700.0, -744.9, A.EXP_CUTOFF, A.nxt(A.EXP_CUTOFF, -1), A.nxt(A.EXP_CUTOFF, 1),
          -746.0, -2.0 ** 100, -0.0, 0.0, 1.0, 709.0, 710.0, math.nan]
    xs += list(-np.random.default_rng(3).uniform(0.0, 750.0, 300))
    for x in xs:
        assert same_bits(A.exp_parts(x)[0], oracle.exp(x)), x


@pytest.mark.parametrize("variant", ["default", "head rotation", "attraction", "sight weights off", "attraction, no sight weights"])
def test_pair_terms_implies_the_oracles_force(oracle, variant):
    """Two pedestrians (one neighbour: no summation order), moving at the reset, eight steps: the force pair_terms implies equals
    the oracle's extra[..., 2:] bit for bit, also in the sign of a zero."""
    sf = {"default": A.default_sf(), "head rotation": A.default_sf(), "attraction": A.default_sf(C=0.25),
          "sight weights off": A.default_sf(sw_use=0.0), "attraction, no sight weights": A.default_sf(C=-0.125, sw_use=0.0)}[variant]
    scenes = []
    for k, (bx, by) in enumerate(((1.5, 0.0), (0.0, -0.75), (-1.25, 2.0), (0.5, 0.5), (-0.0, 1.0), (2.0 ** -40, 0.0))):
        s = A.Scene(f"pin {k}", A.place([A.ped(0.0, 0.0, 4.0, 5.0), A.ped(bx, by, -5.0, 4.0, 1.1)], 2, (0, 1)),
                    vel=None if k % 2 else np.array([[0.5, 0.25], [-0.75, 0.5]]))
        scenes.append(s)
    fam = A.Family("pin", scenes, 2, steps=8, head_rot=0.4 if variant == "head rotation" else 0.0)
    batch = A.pack(fam)
    n = 0
    for r, s in enumerate(scenes):
        o = A.run_oracle(oracle, fam, batch, r, sf)
        assert o["n_steps"] == 8
        for k in range(8):
            for i in range(2):
                assert o["extra"][k + 1, i, 1] == 1.0  # (walking towards its one goal)
                got = implied_force(oracle, fam, o, k, i, sf, s.peds)
                assert same_bits(got, o["extra"][k + 1, i, 2:]), (variant, s.name, k, i, got, o["extra"][k + 1, i, 2:])
                n += 1
    assert n == 6 * 8 * 2


def test_pair_terms_implies_the_force_of_every_scene(oracle, fams, runs):
    """The same on every scene of every small family, with the summation over several neighbours in the oracle's order: the
    guard classification below reads the terms of exactly the pairs the oracle evaluates."""
    n = 0
    for name in SMALL:
        fam = fams[name]
        for pn, sf, res in runs[name][:: max(1, len(runs[name]) // 4)]:
            for r, o in enumerate(res):
                s = fam.scenes[r]
                c = 1 if fam.car else 0
                for k in range(min(o["n_steps"], 2)):
                    for i in {p for pair in s.pairs for p in pair}:
                        if o["extra"][k + 1, i + c, 1] != 1.0:
                            continue
                        got = implied_force(oracle, fam, o, k, i, sf, s.peds)
                        assert same_bits(got, o["extra"][k + 1, i + c, 2:]), (name, pn, s.name, k, i, got, o["extra"][k + 1, i + c, 2:])
                        n += 1
    assert n > 1000, n


def _count(classes, fam, guard, aimed_only=None, step=None):
    n = 0
    for (name, pn, r, k, i, j), (g, _) in classes.items():
        if name == fam and guard in g and (step is None or k == step) and (aimed_only is None or (i, j) in aimed_only(r)):
            n += 1
    return n


def test_every_aimed_pair_trips_its_guard_and_every_twin_trips_nothing(fams, classes):
    twins = 0
    for name in SMALL:
        fam = fams[name]
        for pn, sf in fam.param_sets:
            for r, s in enumerate(fam.scenes):
                for (i, j) in s.pairs:
                    if (s.expect or s.clean) and (name, pn, r, 0, i, j) not in classes:
                        raise AssertionError(f"{name} / {s.name}: the aimed pair {(i, j)} is not active at the first step")
                    if s.expect:
                        g = classes[name, pn, r, 0, i, j][0]
                        assert s.expect <= g, (name, s.name, (i, j), sorted(g))
                    if s.clean:
                        g = classes[name, pn, r, 0, i, j][0]
                        assert not g, (name, s.name, (i, j), sorted(g))
                        twins += 1
    assert twins >= 8, twins  # 2^-50 along x and y, two slot layouts, both directions of the pair


# per family: (guard, the smallest number of (pair, step) evaluations that must trip it).  Written down from the construction:
# near: 3 directions x 5 failing separations (4 on the diagonal) x 2 layouts x 2 directions of the pair = 56 at the first step;
# negzero: 2 axes x 2 mixed sign combinations x 3 speeds x 2 layouts, one direction of the pair = 24 at the first step; ...
AIMED = {
    "near": ("near", 56), "headrot_near": ("near", 28), "headrot_car_near": ("near", 28),
    "negzero": ("negzero", 24), "headrot_negzero": ("negzero", 12), "headrot_car_negzero": ("negzero", 12),
    "faint": ("faint", 2 * 2 * 5),   # 2 layouts x 2 directions x (2 + 3 parameter sets below the crossings)
    "sliver": ("sliver", 3),         # cos_sight = fl(a / m) and both neighbours, for the aimed pair
}


def test_each_family_trips_its_guard(fams, classes, runs):
    got = {name: _count(classes, name, guard, step=0) for name, (guard, _) in AIMED.items()}
    for name, (guard, least) in AIMED.items():
        assert got[name] >= least > 0, (name, guard, got)
    # the cutoff of exp: rep == 0 (the hi word of +0 is below 2^-700) on one side, a finite tiny rep on the other
    zero = sum(1 for (n, pn, r, k, i, j), (g, T) in classes.items() if n == "faint" and k == 0 and T["a_rep"] == 0.0)
    tiny = sum(1 for (n, pn, r, k, i, j), (g, T) in classes.items() if n == "faint" and k == 0 and 0.0 < T["a_rep"] < 2.0 ** -700)
    assert zero >= 16 and tiny >= 8, (zero, tiny)  # (4 parameter sets about the cutoff, 2 below the 2^-700 crossing) x 4 pairs
    either = {pn: sum(1 for (n, q, r, k, i, j), (g, T) in classes.items() if n == "faint" and q == pn and k == 0 and "faint" in g)
              for pn, _ in fams["faint"].param_sets}
    assert either["sigma faint0"] > 0 and either["sigma faint1"] == 0, either  # the two sides of the 2^-700 crossing
    # sliver: the decision is `bad` on the threshold and its neighbours, and decided one double beyond q (1 +- 2^-50)
    sl = {pn: classes["sliver", pn, 0, 0, 0, 1][0] for pn, _ in fams["sliver"].param_sets}
    assert all("sliver" in sl[f"cos_sight {n}"] for n in ("q", "q-1ulp", "q+1ulp")), sl
    decided = [n for n, g in sl.items() if "sliver" not in g]
    assert len(decided) >= 6 + 2, sl  # the six special values, and the outer neighbours of q (1 +- 2^-50)


def test_insane_and_params_guards(oracle, fams, runs):
    fam = fams["insane"]
    (pn, sf, res), = runs["insane"]
    bad = ok = 0
    for s, o in zip(fam.scenes, res):
        P, V = o["poses"][0], o["vels"][0]
        dtn = float(o["t"][1] - o["t"][0])
        for i in range(fam.E):
            v = A.insane(P[i, 0], P[i, 1], V[i, 0], V[i, 1], dtn)
            if i in s.want_insane:
                assert v, (s.name, i)
                bad += 1
            else:
                assert not v, (s.name, i, P[i], V[i])
                ok += i in s.want_sane
    assert bad == 4 * 2 + 1 and ok == 3 * 2, (bad, ok)  # INSANE_COORDS: 4 failing and 3 passing values x 2 axes; the step product
    fam = fams["params"]
    n_bad = 0
    for pn, sf in fam.param_sets:
        assert A.params_bad(sf) == fam.want_params_bad[pn], pn
        n_bad += A.params_bad(sf)
    assert n_bad == 7 and len(fam.param_sets) - n_bad == 6, n_bad
    for name, f in fams.items():  # every other family runs under parameters the crowd kernel accepts
        if name != "params":
            for pn, sf in f.param_sets:
                assert not A.params_bad(sf), (name, pn)


def test_the_only_nan_rows_are_the_listed_ones(fams, runs):
    """Coverage cap: no scene leaves the device comparison because the oracle produced NaN or inf."""
    n_nan = 0
    for name, fam in fams.items():
        c = 1 if fam.car else 0
        for pn, sf, res in runs[name]:
            for s, o in zip(fam.scenes, res):
                assert o["n_steps"] == fam.steps, (name, s.name)
                for key in ("poses", "vels"):
                    for k in range(1, o["n_steps"] + 1):  # every recorded step after the first force (the reset state is the knots')
                        rec = o[key][k][:fam.E + c]
                        rows = np.isnan(rec[:, :2]).any(axis=1) | np.isinf(rec).any(axis=1)
                        assert sorted(np.nonzero(rows)[0] - c) == sorted(s.nan), (name, pn, s.name, key, k, np.nonzero(rows)[0])
                    first = o[key][0][:fam.E + c]  # at the reset only a NaN coordinate that the scene itself put there
                    rows = np.isnan(first[:, :2]).any(axis=1) | np.isinf(first).any(axis=1)
                    assert set(np.nonzero(rows)[0] - c) <= set(s.nan), (name, pn, s.name, key, 0)
                others = np.setdiff1d(np.arange(fam.E), s.nan) + c
                assert not np.isinf(o["extra"][:, others]).any() and not np.isinf(o["dists"][:, others]).any(), (name, s.name)
                n_nan += len(s.nan)
    assert n_nan > 0


# ---- decisiveness without a device ------------------------------------------------------------------------------------------
def _recip(b, ulps=0, steps=2):
    """RecipDiv's reciprocal from an rcp that is `ulps` off the correctly rounded one, `steps` Newton steps."""
    r = A.nxt(A.div(1.0, b), ulps)
    for _ in range(steps):
        r = A.fma(r, A.fma(-b, r, 1.0), r)
    return r


def _recip_div(a, b, r, correct=True):
    q0 = a * r
    return A.fma(A.fma(-b, q0, a), r, q0) if correct else q0


# Lower bounds at half of what the emulation counted when this test was written: q0 only 48 of 672 (midpoint) and 64 of 504
# (midpoint_sigma) operand pairs, slack 0: 6 decisions (the six hard pairs, each under its own threshold).
# "One step short" counts 0 of 672 and 0 of 504, and that 0 is asserted: from an rcp within 1 ulp one Newton step leaves the
# reciprocal within 2^-100 relative, and div's own residual correction squares what error is left in q0 -- on an rcp that
# good the second refinement changes no quotient.  It is there for the hardware's coarser v_rcp_f64, which Python does not have.
MIN_DECISIVE = {("midpoint", "q0 only"): 24, ("midpoint_sigma", "q0 only"): 32, ("sliver", "slack 0"): 3}


def test_wrong_arithmetic_would_show(fams, classes):
    """div without the residual correction; RecipDiv one Newton step short on an rcp that is 1 ulp off; quotient_ge without its
    slack: the number of aimed operands (first step, aimed pairs) whose result is not IEEE's."""
    counts = {}
    for name in ("midpoint", "midpoint_sigma"):
        fam = fams[name]
        n_q0 = n_newton = n_ops = 0
        for (fn, pn, r, k, i, j), (g, T) in classes.items():
            if fn != name or k != 0 or (i, j) not in fam.scenes[r].pairs:
                continue
            for a, b in T["divs"]:
                if not (math.isfinite(a) and math.isfinite(b)) or b == 0.0:
                    continue
                exact = A.div(a, b)
                n_ops += 1
                n_q0 += not same_bits(_recip_div(a, b, _recip(b), correct=False), exact)
                n_newton += any(not same_bits(_recip_div(a, b, _recip(b, u, steps=1)), exact) for u in (-1, 1))
                assert same_bits(_recip_div(a, b, _recip(b)), exact) or A.is_neg_zero(a), (a, b)  # (the sequence itself is right)
        counts[name, "q0 only"], counts[name, "one step short"], counts[name, "operands"] = n_q0, n_newton, n_ops
    n = 0
    for pn, sf in fams["sliver"].param_sets:
        for r, s in enumerate(fams["sliver"].scenes):
            for (i, j) in s.pairs:
                T = classes["sliver", pn, r, 0, i, j][1]
                c = float(sf[A.SF_COS])
                n += (T["a"] >= c * T["m"]) != (A.div(T["a"], T["m"]) >= c)
    counts["sliver", "slack 0"] = n
    for key, least in MIN_DECISIVE.items():
        assert counts[key] >= least > 0, counts
    assert counts["midpoint", "one step short"] == 0 and counts["midpoint_sigma", "one step short"] == 0, counts


# ---- the PID derivative -----------------------------------------------------------------------------------------------------
def _finite(o):
    return all(np.isfinite(o[k][:, 0]).all() for k in ("poses", "vels", "dists", "extra"))


def _pid_live_operands(o, ctrl):
    """The derivative divisions of one PID ego, step by step, from the oracle's record: (step, "lat" / "lon", numerator, State.dt)
    for every division whose numerator is not zero and whose quotient reaches the output -- the steering angle inside
    +-max_steer; the acceleration computed at all (|e_lon| > 0.1) and inside +-max_accel.  PIDController._step restated."""
    t, ex = o["t"], o["extra"][:, 0]
    out = []
    for k in range(o["n_steps"]):
        sdt = 0.1 if k == 0 else float(t[k] - t[k - 1])  # State.dt: prev_t = t - 0.1 at the reset
        speed = ex[k, 0]
        gain = 1.0 - 0.9 * (speed - 5.0) / 10.0 if 5.0 < speed <= 15 else (0.1 if speed > 15 else 1.0)
        e_lon, e_lat, e_int = ex[k + 1, 1], ex[k + 1, 2], ex[k + 1, 3]
        d_lon, d_lat = e_lon - ex[k, 1], e_lat - ex[k, 2]
        steer = ctrl[4] * gain * e_lat + ctrl[5] * gain * A.div(d_lat, sdt)
        accel = ctrl[6] * e_lon + ctrl[7] * A.div(d_lon, sdt) + ctrl[8] * e_int
        if d_lat != 0.0 and abs(steer) < ctrl[0]:
            out.append((k, "lat", float(d_lat), sdt))
        if d_lon != 0.0 and abs(e_lon) > 0.1 and abs(accel) < ctrl[1]:
            out.append((k, "lon", float(d_lon), sdt))
    return out


# lower bounds at half of what was counted when this test was written: live divisions by the all-ones State.dt 36, of them
# decisive (div without its residual correction gives another quotient than IEEE) 20; under the 48-bit timestep 191 live
# divisions, 31 decisive; by the first step's State.dt = 0.1: 20 decisive
PID_MIN = {"ones live": 18, "ones decisive": 10, "48 live": 95, "48 decisive": 15, "0.1 decisive": 10}


def test_pid_scenes_stay_finite_and_reach_their_operands(oracle):
    """The ego's rows stay finite in every PID scene (nothing leaves the device comparison); the moving ego takes the largest
    power-of-two timestep it stays finite under (searched exponent by exponent from 2^600 down, pinned here), the ego at rest
    takes 2^600; "rest" has +0.0 error differences throughout, "lat-0" a first lateral error of -0.0 after a previous one of
    +0.0.  And the rounding-hard divisors reach RecipDiv::div with live numerators: State.dt is t - prev_t, not the timestep, so
    the count is taken from the oracle's own clock -- divisions by the all-ones mantissa (steps 1 and 2 of that timestep), by the
    48-bit timestep (every step from the second) and by the first step's 0.1, each with a non-zero numerator and an output that
    is neither clamped nor switched off, and among them those on which div without its residual correction differs from IEEE."""
    huge = None
    for k in range(600, 0, -1):
        batch, persist = A.pid_pack(2.0 ** k, ("moving",))
        if _finite(A.pid_oracle(oracle, batch, persist, 0, 2.0 ** k)):
            huge = 2.0 ** k
            break
    assert huge == A.PID_HUGE_MOVING, math.log2(huge)
    seen = set()
    counts = dict.fromkeys(PID_MIN, 0)
    for dt, names in A.pid_groups(A.PID_HUGE_MOVING):
        batch, persist = A.pid_pack(dt, names)
        for r, n in enumerate(names):
            o = A.pid_oracle(oracle, batch, persist, r, dt)
            assert o["n_steps"] == A.PID_STEPS and _finite(o), (dt, n)
            seen.add((dt, n))
            if n == "rest":  # on the target at rest: errors (columns 1, 2 of the controller state) and speed stay +0.0
                assert same_bits(o["extra"][:, 0], np.zeros((A.PID_STEPS + 1, 4)))
            if n == "lat-0":
                assert A.is_neg_zero(o["extra"][1, 0, 2]) and A.bits(o["extra"][0, 0, 2]) == 0
            if n == "moving" and dt == A.PID_DT_ONES:  # ordinary, changing errors along and across
                assert np.count_nonzero(np.diff(o["extra"][:, 0, 1])) >= 8 and np.count_nonzero(np.diff(o["extra"][:, 0, 2])) >= 3
            for k, which, a, sdt in _pid_live_operands(o, batch["ctrl"][r * A.PID_E]):
                decisive = not same_bits(_recip_div(a, sdt, _recip(sdt), correct=False), A.div(a, sdt))
                assert same_bits(_recip_div(a, sdt, _recip(sdt)), A.div(a, sdt))
                key = "ones" if sdt == A.PID_DT_ONES else ("48" if sdt == A.PID_DT_48 else None)
                if key:
                    counts[key + " live"] += 1
                    counts[key + " decisive"] += decisive
                if sdt == 0.1:
                    counts["0.1 decisive"] += decisive
    assert len(seen) == 13 + 8 + 9
    for key, least in PID_MIN.items():
        assert counts[key] >= least > 0, counts


def test_noise_scene_reaches_the_small_f_branch_of_log(oracle):
    """The committed (seed, entity, step) put a uniform within 2^-20 of a power of two: the Philox restatement is the oracle's (its
    Box-Muller pair, rebuilt from the two uniforms with the oracle's log and sincos, equals sgo_noise_pair bit for bit), the
    uniform is the committed one, sgo_log's first test is true for it -- with both signs of f and both of its return forms --
    and the pedestrian is walking at that step, so the scene draws that pair."""
    fam = A.log_family()
    batch = A.pack(fam)
    forms = set()
    for seed, ent, step, u in A.LOG_SMALL_F:
        u1, u2 = A.philox_uniforms(seed, 0, ent, step)
        assert u1 == u and A.log_takes_small_f_branch(u1)
        r = math.sqrt(-2.0 * oracle.log(u1))
        sn, cs = oracle.sincos(6.28318530717958623200e+00 * u2)
        assert same_bits([r * cs, r * sn], oracle.noise_pair(seed, 0, ent, step))
        forms.add(u1 > 0.75)
        o = A.run_oracle(oracle, fam, batch, 0, A.default_sf(), noise=dict(mode="device", std_lon=A.LOG_STD[0], std_lat=A.LOG_STD[1],
                                                                            seed=seed, scenario_index=0))
        assert o["extra"][step + 1, ent, 1] == 1.0 and np.isfinite(o["poses"][:, :fam.E, :2]).all()
        quiet = A.run_oracle(oracle, fam, batch, 0, A.default_sf())
        assert not same_bits(o["poses"][step + 1, ent], quiet["poses"][step + 1, ent])  # (the variates moved it)
    assert forms == {True, False}
    n = sum(A.log_takes_small_f_branch(A.philox_uniforms(7, 0, e, s)[0]) for e in range(64) for s in range(64))
    assert n == 0  # (an ordinary seed does not get there in 4,096 draws)
